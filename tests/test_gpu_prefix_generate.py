"""generate(prefix=...) on the GPU: detached prefixes (snapshot, persistence, detached scoring), the placement of a prefix under
its decode rows bit for bit, and the prefill / decode / generate behind a prefix against the plain path on the concatenated prompts
(the reference's golden ids included).  Bounds are the project's own for the same positions through another launch shape
(DESIGN.md section 3); observed figures go through gpu_helpers.record (those of the MI355X run are committed as
profiles/prefix_generate_parity.jsonl)."""
import json
import os

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth
import forward_checks as fc
import gen_scores_checks as gsc
import prefix_generate_checks as pg
from gpu_helpers import record, rel_l2

pytestmark = pytest.mark.gpu

MICRO_REL_L2 = 1.5e-2          # micro models (tests/test_gpu_parity.py REL_L2)
ROW_VS_BATCH_LOGITS = 3e-3     # Llama-3-8B widths: a row of the batch vs that row alone (tests/test_gpu_batch64.py)
GEMM_KV = 2e-3                 # projection output against another GEMM route, of max|ref|
DECODE_VS_PREFILL = 1.5e-2     # token_logprobs vs score_continuations (tests/test_gpu_nsamples.py)
DECISIVE_MIN = 0.9
# (preset, prefix lengths, suffix lengths, row map, seed): seeds chosen on the CPU oracle so that >= 90 % of the steps are decisive
GREEDY_CASES = {
    "micro": ("micro", [9, 14, 5], [6, 1, 11, 4, 8], [2, 0, 0, 1, 2], 1),
    "micro_qwen": ("micro_qwen", [9, 14, 5], [6, 1, 11, 4, 8], [2, 0, 0, 1, 2], 1),
    "micro_opt": ("micro_opt", [9, 14, 5], [6, 1, 11, 4, 8], [2, 0, 0, 1, 2], 4),
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def micro(dev):
    return fc.make_model(opa.micro(), dev)


# ------------------------------------------------------------------------------------------------ exact
def test_snapshot_equals_a_second_export_and_outlives_a_generate(micro):
    model, cfg = micro, micro.cfg
    pre, _, _ = pg.text_batch(cfg, [7, 12, 3], [1], [0], seed=3)
    pids, pmask = pg.left_pad(pre)
    live = model.cache_prefix(pids, attention_mask=pmask)
    assert not live.detached and live.slots == 12 and live.rows == 3
    det = pg.live_copy_detached(live)
    k, v, kst = model.export_cache(live._epoch, 3, 12)
    assert det.detached and pg.same(det._k, k) and pg.same(det._v, v) and torch.equal(det._kstart, kst)
    assert kst.tolist() == [5, 0, 9] and tuple(k.shape) == (cfg.dec_layers, 3, cfg.dec_kv_heads, 12, cfg.dec_head_dim)
    assert k.dtype == _cabi.operand_dtype() and float(k.float().abs().max()) > 0
    cc = _cabi.CConfig.from_config(cfg)
    import ctypes as C
    assert k.numel() * 2 + v.numel() * 2 == model._lib.opus_llama_prefix_bytes(C.byref(cc), 3, 12)
    k0, v0 = det._k.clone(), det._v.clone()
    ids, mask, seqs = gsc.batch(cfg, 4)
    model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=4)
    assert pg.same(det._k, k0) and pg.same(det._v, v0)
    with pytest.raises(_cabi.OpusError) as e:                     # the live handle is stale now: no export, no detach
        model.export_cache(live._epoch, 3, 12)
    assert e.value.code == -6
    with pytest.raises(_cabi.OpusError) as e:
        live.detach()
    assert e.value.code == -6 and not live.detached
    assert model.cache_prefix(pids, attention_mask=pmask, detach=True).detached
    record("prefix_generate.snapshot", dict(equals_second_export=True, unchanged_by_generate=True, stale_live_code=-6, bytes=k.numel() * 4))


@pytest.mark.parametrize("hd,nh,nkv", pg.PLACE_SHAPES)
def test_placement_bit_for_bit(dev, hd, nh, nkv):
    o = pg.placement(dev, hd, nh, nkv)
    record(f"prefix_generate.placement.hd{hd}_kv{nkv}", o)
    assert len(o) == 4 and all(c["block"] and c["sentinel"] and c["kstart"] for c in o.values()), o


def test_fan_out_rows_are_bit_identical(micro):
    model, cfg = micro, micro.cfg
    pre, suf, _ = pg.text_batch(cfg, [11, 6], [5, 5, 3], [1, 1, 0], seed=5)
    suf[1] = suf[0]                                                # rows 0 and 1: the same prefix row, the same suffix
    pids, pmask = pg.left_pad(pre)
    prefix = model.cache_prefix(pids, attention_mask=pmask, detach=True)
    emb, _ = pg.embed(model, *pg.right_pad(suf), left=False)
    lg, _ = model.prefill_logits_behind(prefix, emb, [5, 5, 3], [1, 1, 0])
    assert pg.same(lg[0], lg[1]) and not pg.same(lg[0], lg[2])
    for _ in range(3):
        tok = lg.argmax(dim=1)
        tok[1] = tok[0]
        lg = model.decode_logits(tok)
        assert pg.same(lg[0], lg[1]) and not pg.same(lg[0], lg[2])
    record("prefix_generate.fan_out", dict(rows_bit_identical=True, steps=3))


def test_detached_handle_persists_and_moves_to_a_new_context(micro):
    model, cfg = micro, micro.cfg
    pre, suf, _ = pg.text_batch(cfg, [9, 14, 5], [6, 1, 11, 4], [2, 0, 0, 1], seed=8)
    pids, pmask = pg.left_pad(pre)
    prefix = model.cache_prefix(pids, attention_mask=pmask, detach=True)
    sids, smask = pg.left_pad(suf)
    kw = dict(attention_mask=smask, prefix=prefix, prefix_rows=[2, 0, 0, 1], pad_token_id=2, max_new_tokens=6,
              return_dict_in_generate=True, output_token_logprobs=True)
    a = model.generate(sids, **kw)
    ids, mask, seqs = gsc.batch(cfg, 5, seed=1)
    model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=5)       # unrelated, overwrites the cache
    b = model.generate(sids, **kw)
    assert torch.equal(a.sequences, b.sequences) and pg.same(a.token_logprobs, b.token_logprobs)
    other = model.new_context()
    c = other.generate(sids, **kw)
    assert torch.equal(a.sequences, c.sequences) and pg.same(a.token_logprobs, c.token_logprobs)
    assert other.stat("prefills_behind") == 1 and model.stat("prefills_behind") >= 2
    # a live handle is detached on the fly (one export) and is stale afterwards
    live = model.cache_prefix(pids, attention_mask=pmask)
    d = model.generate(sids, **dict(kw, prefix=live))
    assert live.detached and torch.equal(d.sequences, a.sequences) and pg.same(d.token_logprobs, a.token_logprobs)
    record("prefix_generate.persistence", dict(same_handle_twice=True, new_context=True, live_detached_on_the_fly=True))


def test_detached_scoring_equals_live_scoring(micro):
    from opus_pllm_amd.constraint import TokenTrie
    model, cfg = micro, micro.cfg
    pre, conts, _ = pg.text_batch(cfg, [9, 14, 5], [6, 1, 8, 4, 3], [2, 0, 0, 1, 2], seed=9)
    src = torch.tensor([2, 0, 0, 1, 2])
    conts = [torch.from_numpy(c) for c in conts]
    trie = TokenTrie([[10, 11], [10, 12, 13], [14], [15, 16, 17]], end_token_id=1)
    pids, pmask = pg.left_pad(pre)
    live = model.cache_prefix(pids, attention_mask=pmask)
    a = model.score_continuations(live, conts, prefix_rows=src)
    ta = model.score_trie(live, trie, include_stop=True)
    det = pg.live_copy_detached(live)
    b = model.score_continuations(det, conts, prefix_rows=src)
    tb = model.score_trie(det, trie, include_stop=True)
    assert pg.same(a.token_logprobs, b.token_logprobs) and pg.same(ta.member_logprob, tb.member_logprob)
    assert pg.same(ta.stop_logprob, tb.stop_logprob) and pg.same(ta.node_logprobs, tb.node_logprobs)
    ids, mask, seqs = gsc.batch(cfg, 4)
    model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=4)       # the live handle goes stale
    c = model.score_continuations(det, conts, prefix_rows=src)
    tc = model.score_trie(det, trie, include_stop=True)
    assert pg.same(a.token_logprobs, c.token_logprobs) and pg.same(ta.member_logprob, tc.member_logprob)
    for call in (lambda: model.score_continuations(live, conts, prefix_rows=src), lambda: model.score_trie(live, trie)):
        with pytest.raises(_cabi.OpusError) as e:
            call()
        assert e.value.code == -6
    d = model.new_context().score_continuations(det, conts, prefix_rows=src)
    assert pg.same(a.token_logprobs, d.token_logprobs)
    record("prefix_generate.detached_scoring", dict(continuations_bitwise=True, trie_bitwise=True, after_stale=True, new_context=True))


def test_no_decode_graph_of_its_own(micro):
    model, cfg = micro, micro.cfg
    model.drop_decode_graphs()
    pre, suf, cat = pg.text_batch(cfg, [9, 14], [6, 2, 7], [1, 0, 0], seed=10)
    cids, cmask = pg.left_pad(cat)
    kw = dict(pad_token_id=2, max_new_tokens=6)
    model.generate(cids, attention_mask=cmask, **kw)                # a plain 3-row batch creates the entry
    i0, n0, r0 = model.stat("graph_instantiations"), model.stat("graphs_cached"), model.stat("graph_replays")
    assert n0 == 1
    pids, pmask = pg.left_pad(pre)
    prefix = model.cache_prefix(pids, attention_mask=pmask, detach=True)
    sids, smask = pg.left_pad(suf)
    model.generate(sids, attention_mask=smask, prefix=prefix, prefix_rows=[1, 0, 0], **kw)
    assert model.stat("graph_instantiations") == i0 and model.stat("graphs_cached") == n0
    assert model.stat("graph_replays") > r0
    record("prefix_generate.graph_cache", dict(new_instantiations=model.stat("graph_instantiations") - i0, graphs_cached=n0))


# ------------------------------------------------------------------------------------------------ the reference's golden ids
@pytest.mark.parametrize("how", ["behind_seq", "before_seq", "last_token"])
def test_generate_micro_golden_ids_behind_a_prefix(micro, gold, gold_dir, how):
    """tests/test_gpu_parity.py::test_generate_micro_golden_ids demands every id of the fixture (no low-margin step) and the
    EOS-then-pad rows of the plain call: the same of the call split at three places."""
    model = micro
    g = gold("generate_micro")
    seqs = json.load(open(os.path.join(gold_dir, "generate_micro.seqs.json")))
    pad, eos, N = int(g["pad"]), int(g["eos"]), g["free_ids"].shape[1]
    pre, suf = pg.cut_rows(g["ids"], g["mask"], how)
    pids, pmask = pg.left_pad(pre)
    sids, smask = pg.left_pad(suf)
    in_prefix = how != "before_seq"                                  # which side holds the protein
    prefix = model.cache_prefix(pids, seqs if in_prefix else None, attention_mask=pmask, detach=True)
    kw = dict(attention_mask=smask, prefix=prefix, pad_token_id=pad, do_sample=False, max_new_tokens=N)
    if not in_prefix:
        kw["seq"] = seqs
    out = model.generate(sids, **kw)
    assert out.dtype == torch.long and np.array_equal(out.cpu().numpy(), g["free_ids"]), (how, out)
    out2 = model.generate(sids, eos_token_id=[eos], **kw)
    assert np.array_equal(out2.cpu().numpy(), g["eos_ids_out"]), (how, out2)
    assert torch.equal(model.generate(sids, **kw), out)             # graph replay


@pytest.mark.parametrize("tag,preset", [("generate_micro_opt", "micro_opt"), ("generate_micro_opt_relu", "micro_opt_relu"),
                                        ("generate_micro_qwen", "micro_qwen")])
def test_decoder_family_golden_behind_a_prefix(dev, gold, tag, preset):
    """tests/test_gpu_parity.py::test_decoder_family_golden demands every greedy id of the family fixtures and REL_L2 on the
    prefill + 4 teacher-forced steps: the same of the three cuts of the spliced rows."""
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    cfg = opa.PRESETS[preset]()
    base, g = gold("generate_micro"), gold(tag)
    canon = synth.canonical_weights(cfg, int(g["weights_seed"]))
    model = OpusLlamaForCausalLM(cfg, DeviceWeights.from_canonical(cfg, canon, dev), dev)
    emb, mask = torch.from_numpy(base["embeds"]).half(), torch.from_numpy(base["mask_out"]).bool()
    ref, free = torch.from_numpy(g["step_logits"]), torch.from_numpy(g["free_ids"])
    obs = {}
    for how in ("behind_seq", "before_seq", "last_token"):
        pe, pm, se, lens = pg.cut_embeds(emb, mask, base["ids"], base["mask"], cfg.n_prot_tokens, how)
        prefix = pg.prefix_from_embeds(model, pe, pm)
        lg, _ = model.prefill_logits_behind(prefix, se, lens)
        rel = [rel_l2(lg, ref[:, 0])]
        for s in range(4):
            lg = model.decode_logits(free[:, s]).cpu()
            rel.append(rel_l2(lg, ref[:, s + 1]))
            assert torch.equal(lg.argmax(-1), ref[:, s + 1].argmax(-1)), (how, s)
        out = pg.greedy_behind_embeds(model, prefix, se, lens, free.shape[1])
        obs[how] = dict(rel_l2=rel, ids_equal=bool(torch.equal(out.cpu(), free)))
    record(f"prefix_generate.family.{tag}", obs)
    for how, o in obs.items():
        assert max(o["rel_l2"]) < MICRO_REL_L2 and o["ids_equal"], (how, o)


# ------------------------------------------------------------------------------------------------ logits and K / V vs the plain path
LOGIT_CASES = {
    # T' = 63 .. 66 with 4 decode steps: the steps open a new 32-slot key tile at slot 64 (T' + step - 1 reaches 66 .. 69)
    "tile_63": ([40, 33, 21], [23, 9, 23, 1], [0, 1, 2, 0]),
    "tile_64": ([40, 33, 21], [24, 9, 24, 1], [0, 1, 2, 0]),
    "tile_65": ([40, 33, 21], [25, 9, 25, 1], [0, 1, 2, 0]),
    "tile_66": ([40, 33, 21], [26, 9, 26, 1], [0, 1, 2, 0]),
    # ragged prefixes and ragged suffixes together, repeated / permuted / unused prefix rows, R > P
    "ragged": ([9, 31, 2, 17], [6, 1, 11, 4, 8, 13, 2], [2, 0, 0, 1, 2, 2, 0]),
}


@pytest.mark.parametrize("preset", ["micro", "micro_qwen", "micro_opt"])
def test_logits_and_suffix_kv_vs_plain_prefill(dev, preset):
    cfg = getattr(opa, preset)(max_prompt=72)          # (72 + 16 new tokens: inside micro_opt's 96 learned positions)
    model = fc.make_model(cfg, dev)
    for name, (plens, slens, src) in LOGIT_CASES.items():
        o = pg.logits_vs_plain(model, plens, slens, src, seed=len(name))
        record(f"prefix_generate.logits.{preset}.{name}", o)
        if name.startswith("tile_"):
            assert o["T_new"] == int(name[5:]) and o["last_slot"] >= 64
        assert max(o["rel_l2"]) < MICRO_REL_L2, (name, o)
        assert o["kv_layer0"] < GEMM_KV, (name, o)


def test_llama3_8b_widths_12_rows_behind_3_prefixes(dev):
    cfg = gsc.llama8b_shape(16, 2, 8)
    model = fc.make_model(cfg, dev)
    src = [0, 1, 2] * 4
    o = pg.logits_vs_plain(model, [21, 14, 9], [6 + (5 * i) % 11 for i in range(12)], src, seed=4)
    record("prefix_generate.logits.llama8b_2layer", o)
    assert max(o["rel_l2"]) < ROW_VS_BATCH_LOGITS, o
    assert o["kv_layer0"] < GEMM_KV, o
    del model
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ generate() vs the plain call
@pytest.mark.parametrize("name", list(GREEDY_CASES))
def test_greedy_ids_and_token_logprobs(dev, name):
    preset, plens, slens, src, seed = GREEDY_CASES[name]
    model = fc.make_model(getattr(opa, preset)(), dev)
    plain, behind, prefix, suf = pg.gen_pair(model, plens, slens, src, seed)
    o = pg.decisive_compare(behind.sequences, plain.sequences, plain.logits)
    # token_logprobs of the scored generate, teacher-forced two ways: behind the cached concatenation (prefix + suffix as one
    # plain prefill, the generated ids as the continuation), and behind the detached prefix itself with suffix + generated ids as
    # the continuation (its tail positions)
    _, _, cat = pg.text_batch(model.cfg, plens, slens, src, seed)
    cids, cmask = pg.left_pad(cat)
    whole = model.cache_prefix(cids, attention_mask=cmask)
    sc = model.score_continuations(whole, behind.sequences.cpu())
    o["teacher_forced_abs"] = float((behind.token_logprobs.cpu() - sc.token_logprobs.cpu()).abs().max())
    gen = behind.sequences.cpu()
    sc2 = model.score_continuations(prefix, [torch.cat([torch.from_numpy(x), gen[r]]) for r, x in enumerate(suf)], prefix_rows=src)
    tail = torch.stack([sc2.token_logprobs[r, len(x): len(x) + gen.shape[1]].cpu() for r, x in enumerate(suf)])
    o["teacher_forced_prefix_abs"] = float((behind.token_logprobs.cpu() - tail).abs().max())
    o["vs_plain_lp_abs"] = float((behind.token_logprobs.cpu() - plain.token_logprobs.cpu()).abs().max()) if o["ids_equal"] and \
        o["decisive"] == 1.0 else None
    record(f"prefix_generate.greedy.{name}", o)
    assert o["decisive"] >= DECISIVE_MIN, o
    assert o["ids_equal"], (o, behind.sequences, plain.sequences)
    assert o["teacher_forced_abs"] < DECODE_VS_PREFILL and o["teacher_forced_prefix_abs"] < DECODE_VS_PREFILL, o


def test_features_behind_a_prefix(micro):
    """A TokenTrie, a repetition penalty, a stop sequence and sampling with a seed, each behind a prefix against its plain call."""
    from opus_pllm_amd.constraint import TokenTrie
    model = micro
    _, plens, slens, src, seed = GREEDY_CASES["micro"]
    obs = {}
    trie = TokenTrie([[10, 11], [10, 12, 13], [14], [15, 16, 17]], end_token_id=1)
    plain, behind, _, _ = pg.gen_pair(model, plens, slens, src, seed, max_new=6, prefix_allowed_tokens_fn=trie, eos_token_id=[1])
    obs["trie"] = pg.decisive_compare(behind.sequences, plain.sequences, plain.scores)
    members = [[10, 11], [10, 12, 13], [14], [15, 16, 17]]
    for row in behind.sequences.cpu().tolist():
        assert 1 in row and row[: row.index(1)] in members, row
    model._set_token_constraint(None)
    plain, behind, _, _ = pg.gen_pair(model, plens, slens, src, seed, repetition_penalty=1.3)
    obs["repetition_penalty"] = pg.decisive_compare(behind.sequences, plain.sequences, plain.scores)
    model._set_logits_processors(None)
    free, _, _, _ = pg.gen_pair(model, plens, slens, src, seed)
    stop = free.sequences[0, 2:4].tolist()                            # row 0 stops behind its 4th token
    plain, behind, _, _ = pg.gen_pair(model, plens, slens, src, seed, stop_sequence=stop)
    obs["stop_sequence"] = pg.decisive_compare(behind.sequences, plain.sequences, plain.scores)
    assert bool((behind.sequences[0, 4:] == pg.PAD).all()) and behind.sequences[0, 2:4].tolist() == stop
    model.set_stop_sequence(None)
    mode = dict(temperature=1.0, top_p=0.9, top_k=50)
    plain, behind, prefix, suf = pg.gen_pair(model, plens, slens, src, seed, do_sample=True, seed=77, **mode)
    obs["sampling"] = pg.draws_follow_fp64_rule(behind, mode, 77)
    sids, smask = pg.left_pad(suf)
    kw = dict(attention_mask=smask, prefix=prefix, prefix_rows=src, pad_token_id=2, max_new_tokens=8, do_sample=True, **mode)
    again = model.generate(sids, seed=77, **kw)
    obs["sampling"]["same_seed_equal"] = bool(torch.equal(again, behind.sequences))
    many = model.generate(sids[:2], **dict(kw, attention_mask=smask[:2], prefix_rows=src[:2], seed=78, num_return_sequences=3,
                                           return_dict_in_generate=True, output_logits=True, output_token_logprobs=True))
    obs["sampling"]["nret_rows"] = int(many.sequences.shape[0])
    # rows r N + j: every draw is the fp64 rule's for its decoder row index, and a row's N answers are not all the same
    obs["nret"] = pg.draws_follow_fp64_rule(many, mode, 78)
    m3 = many.sequences.view(2, 3, -1)
    obs["nret"]["replicas_all_equal"] = bool(all(bool((m3[b] == m3[b, :1]).all()) for b in range(2)))
    record("prefix_generate.features", obs)
    for k in ("trie", "repetition_penalty", "stop_sequence"):
        assert obs[k]["ids_equal"] and obs[k]["decisive"] >= 0.5, (k, obs[k])
    s = obs["sampling"]
    assert s["mismatches"] == 0 and s["inadmissible"] == 0 and s["draws"] >= 30 and s["same_seed_equal"] and s["nret_rows"] == 6, s
    t = obs["nret"]
    assert t["mismatches"] == 0 and t["inadmissible"] == 0 and t["draws"] == 48 and not t["replicas_all_equal"], t


def test_api_errors(micro):
    model, cfg = micro, micro.cfg
    pre, suf, _ = pg.text_batch(cfg, [9, 14], [6, 2], [0, 1], seed=2)
    pids, pmask = pg.left_pad(pre)
    prefix = model.cache_prefix(pids, attention_mask=pmask, detach=True)
    sids, smask = pg.left_pad(suf)
    kw = dict(prefix=prefix, pad_token_id=2, max_new_tokens=4)
    with pytest.raises(NotImplementedError):
        model.generate(sids, attention_mask=smask, num_beams=2, **kw)
    empty = smask.clone()
    empty[1] = False
    with pytest.raises(ValueError, match="row 1 is empty"):
        model.generate(sids, attention_mask=empty, **kw)
    with pytest.raises(ValueError, match="pass prefix_rows"):
        model.generate(sids[:1], attention_mask=smask[:1], **kw)
    long = torch.full((2, cfg.max_prompt - 14 + 1), 5)
    with pytest.raises(_cabi.OpusError, match=r"14 slots \+ suffix of 35 positions = 49.*max_prompt=48") as e:
        model.generate(long, **kw)
    assert e.value.code == -2
    with pytest.raises(_cabi.OpusError, match="9 decoder rows.*max_batch=8") as e:
        model.generate(sids[:1].repeat(9, 1), attention_mask=smask[:1].repeat(9, 1), prefix_rows=[0] * 9, **kw)
    assert e.value.code == -2
    # the native checks say the same to a caller of the C entry
    import ctypes as C
    emb, _ = pg.embed(model, *pg.right_pad([np.full(35, 5), np.full(35, 5)]), left=False)
    with pytest.raises(_cabi.OpusError) as e:
        model.prefill_logits_behind(prefix, emb, [35, 35])
    assert e.value.code == -2
    emb, _ = pg.embed(model, *pg.right_pad(suf), left=False)
    with pytest.raises(_cabi.OpusError) as e:
        model.prefill_logits_behind(prefix, emb, [6, 0])
    assert e.value.code == -2
    assert model.generate(sids, attention_mask=smask, **kw).shape == (2, 4)     # and the context still works


# ------------------------------------------------------------------------------------------------ the driver
def test_eval_loop_share_prompt_head():
    """eval_ddp.annotate(share_prompt_head=True) (--share_prompt_head) on the synthetic tokenizer: one cache_prefix per shard, every
    batch generated behind it, and the ids of the run without the flag on the steps its own logits decide."""
    import importlib.util
    from opus_pllm_amd import builder
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(root, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    tok, model, _ = builder.load_pretrained_model("synthetic:c1_tiny", "synthetic", "c1_tiny", device="cuda:0", max_batch=4,
                                                  max_enc_tokens=258, max_prompt=64, max_new_tokens=8)
    items = [dict(instruction=f"What is the function of protein {i}?", input=synth.synth_protein(20 + 11 * (i % 9), i), output="x")
             for i in range(7)]
    rows = [opa.tokenizer_seq_token(ddp.build_prompt(q["instruction"], ""), tok, opa.DEFAULT_SEQ_TOKEN_INDEX) for q in items]
    head_len = ddp.shared_head_length(rows)
    assert head_len >= 1 and all(list(r[:head_len]) == list(rows[0][:head_len]) for r in rows)
    assert all(opa.DEFAULT_SEQ_TOKEN_INDEX not in list(r[:head_len]) for r in rows)
    orig, logits = model.generate, []

    def spy(*a, **k):                                  # the plain run's per-step logits, for its own margins
        out = orig(*a, **dict(k, return_dict_in_generate=True, output_logits=True))
        logits.append(out.logits)
        return out.sequences
    model.generate = spy
    plain = ddp.annotate(model, tok, items, "", 4, 8)
    model.generate = orig
    calls = []
    model.generate = lambda *a, **k: (calls.append(k), orig(*a, **k))[1]
    cached, orig_cache = [], model.cache_prefix
    model.cache_prefix = lambda *a, **k: (cached.append(k), orig_cache(*a, **k))[1]
    b0 = model.stat("prefills_behind")
    shared = ddp.annotate(model, tok, items, "", 4, 8, share_prompt_head=True)
    model.generate, model.cache_prefix = orig, orig_cache
    assert len(cached) == 1 and cached[0].get("detach") is True and model.stat("prefills_behind") == b0 + 2
    assert len(calls) == 2 and all(k["prefix"] is calls[0]["prefix"] and k["prefix"].detached and k["prefix"].rows == 1 for k in calls)
    assert calls[0]["prefix"].slots == head_len
    obs, at = {"head_len": head_len, "batches": []}, 0
    for lg in logits:
        n = lg[0].shape[0]
        w = len(lg)
        obs["batches"].append(pg.decisive_compare(shared[at: at + n, :w], plain[at: at + n, :w], lg))
        at += n
    record("prefix_generate.driver", obs)
    assert at == 7 and all(b["ids_equal"] for b in obs["batches"]), (obs, shared, plain)
    assert min(b["decisive"] for b in obs["batches"]) >= 0.5, obs
    # it composes with sampling and several answers per item: 2 prompts x 2 answers per call
    torch.manual_seed(3)
    many = ddp.annotate(model, tok, items[:4], "", 4, 8, temperature=0.9, top_p=0.95, num_return_sequences=2, share_prompt_head=True)
    assert many.shape == (8, 8)
