"""FP8 decoder weights on the GPU: the load-time quantiser against its CPU twin (bit for bit), every GEMM cell of the skinny, mid,
wide and stream kernels with the FP8 form of W (route unchanged, FP8 panels streamed, exact result), the fall-back of the classes
without an FP8 form (ring, tile, pp), Gaussian operands with the row exponents spread inside a panel and inside a gate / up pair, and the FP8 model against the model
of the same dequantised weights without FP8 tensors (decoder_weights="fp8_dequantized").

Observed figures of a run: profiles/w8_parity.jsonl.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth
from opus_pllm_amd.constraint import TokenTrie
from opus_pllm_amd.model import OpusLlamaForCausalLM
from opus_pllm_amd.weights import DeviceWeights, quantize_fp8, untile_fp8, untile_weight
import gemm_cells_checks as K
import gemm_cells_ref as R
import w8_checks as Q
import w8_ref as W8
from gpu_helpers import record, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_TAU = 0.05
DECODE_BOUND = 2e-3                # tests/test_gpu_batch64.py: decode step vs prefill of the longer prompt


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx(dev):
    cfg = opa.llama3_8b(max_batch=64, max_enc_tokens=1026, max_prompt=104, max_new_tokens=16)
    c = K.make_ctx(cfg, dev)
    yield c
    _cabi.check(_cabi.lib().opus_check_error(c, None))
    _cabi.lib().opus_ctx_destroy(c)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 2. the quantiser
def _weights(N, Kk, dt, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, Kk, generator=g) * torch.logspace(-3, 2, N)[torch.randperm(N, generator=g)][:, None]).to(dt)
    edge = W8.edge_rows(Kk, dt)
    n = min(len(edge), N)
    W[:n] = edge[:n]                                              # the rules' edges, planted
    return W


def _check_quantiser(W, dev):
    q_ref, e_ref, dq_ref = W8.quantize(W)
    q8, e8, dq = quantize_fp8(W.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(e8.cpu(), e_ref)
    assert torch.equal(untile_fp8(q8).cpu(), q_ref)
    assert torch.equal(q8.cpu(), W8.tile(q_ref))
    assert torch.equal(K._bits(dq.cpu()), K._bits(dq_ref))
    assert not ((q8 & 0x7f) == 0x7f).any()


@pytest.mark.parametrize("N,Kk", [(16, 64), (48, 192), (4096 + 16, 1088)])
def test_quantiser_is_the_twin_bit_for_bit(dev, N, Kk):
    _check_quantiser(_weights(N, Kk, _cabi.operand_dtype(), N + Kk), dev)


def test_quantiser_on_gate_up_interleaved_rows(dev):
    """[64, 128] as the loader interleaves gate and up: 32-row groups [16 gate | 16 up], the two halves on different scales."""
    dt = _cabi.operand_dtype()
    g = torch.Generator().manual_seed(3)
    gate, up = torch.randn(32, 128, generator=g) * 0.5, torch.randn(32, 128, generator=g) * 2.0 ** -7
    W = torch.empty(64, 128)
    W.view(2, 2, 16, 128)[:, 0] = gate.view(2, 16, 128)
    W.view(2, 2, 16, 128)[:, 1] = up.view(2, 16, 128)
    _check_quantiser(W.to(dt), dev)
    e = W8.row_exponents(W.to(dt)).view(2, 2, 16)
    assert int((e[:, 0].float().mean() - e[:, 1].float().mean()).abs()) >= 5


def test_quantiser_in_place_and_refusals(dev):
    dt = _cabi.operand_dtype()
    W = _weights(32, 128, dt, 9).to(dev)
    q8, e8, dq = quantize_fp8(W)
    q2, e2 = torch.empty_like(q8), torch.empty_like(e8)
    W2 = W.clone()
    _cabi.check(_cabi.lib().opus_quantize_fp8(W2.data_ptr(), 32, 128, q2.data_ptr(), e2.data_ptr(), W2.data_ptr(), None))   # dq over src
    assert torch.equal(K._bits(W2), K._bits(dq)) and torch.equal(q2, q8) and torch.equal(e2, e8)
    for bad in (float("nan"), float("inf"), -float("inf")):
        Wb = W.clone()
        Wb[17, 77] = bad
        with pytest.raises(_cabi.OpusError, match="not finite"):
            quantize_fp8(Wb)
    lib = _cabi.lib()
    assert lib.opus_quantize_fp8(W.data_ptr(), 24, 128, q2.data_ptr(), e2.data_ptr(), None, None) == -2      # N % 16
    assert lib.opus_quantize_fp8(W.data_ptr(), 32, 96, q2.data_ptr(), e2.data_ptr(), None, None) == -2       # K % 64
    assert lib.opus_quantize_fp8(None, 32, 128, q2.data_ptr(), e2.data_ptr(), None, None) == -1


# ------------------------------------------------------------------------------------------------ 3. cells
ALL = R.CASES + R.SLAB_CASES
W8_CASES = [c for c in ALL if R.route_case(c) is not None and R.route_case(c).klass in Q.W8_CLASSES]


def _first(klass):
    return next(c for c in ALL if c.plan.klass == klass and c.M * c.N * c.K < 1 << 28)


# one case of every class without an FP8 form: the launch reads the fp16 copy
FALLBACK_CASES = [_first(k) for k in (R.RING, R.TILE)] + [next(c for c in ALL if c.plan.klass == R.PP)]


def test_case_tables():
    assert len(W8_CASES) >= 150 and all(c.plan.klass in Q.W8_CLASSES for c in W8_CASES)
    assert len(W8_CASES) == len([c for c in ALL if c.plan.klass in (R.SKINNY, R.MID, R.WIDE, R.STREAM)])
    cells = {R.cell_of(c) for c in W8_CASES}
    # every cell of the four weight-streaming classes (fused norm, k-parts through either reduce, in-launch combine, the slab forms)
    assert cells == {c for c in R.CELLS + R.SLAB_CELLS if c.klass in Q.W8_CLASSES}
    assert all(c.plan.klass not in Q.W8_CLASSES for c in FALLBACK_CASES)


@pytest.mark.parametrize("c", W8_CASES, ids=R.case_id)
def test_w8_cell_routes_as_before_and_is_exact(ctx, dev, c):
    assert R.route_case(c) == c.plan
    obs = Q.run_exact_case(ctx, dev, c, repeats=K.REPEATS if c.plan.combine == R.IN_LAUNCH else 2)
    if "exact" not in obs:
        print("w8_cells", obs["id"], "err", obs["err"], "ref_max", obs["ref_max"], "bound", K.bound(c, obs))
        record("w8_cells." + obs["id"], {"err": obs["err"], "ref_max": obs["ref_max"], "bound": K.bound(c, obs)})
    bad = Q.failures(c, obs)
    assert not bad, (obs["id"], bad)


@pytest.mark.parametrize("c", FALLBACK_CASES, ids=R.case_id)
def test_class_without_fp8_form_reads_the_fp16_copy(ctx, dev, c):
    obs = Q.run_exact_case(ctx, dev, c)
    assert obs["ran_w8"] == [0]
    bad = Q.failures(c, obs)
    assert not bad, (obs["id"], bad)


# ------------------------------------------------------------------------------------------------ 4. Gaussian operands
def _case(M, N, Kk, epi, mode, norm, a_tiled=False):
    return next(c for c in R.CASES if (c.M, c.N, c.K, c.epi, c.mode, c.norm, c.a_tiled) == (M, N, Kk, epi, mode, norm, a_tiled))


GAUSS = [_case(1, 200, 192, R.PLAIN, R.F16, False), _case(1, 200, 192, R.GELU, R.F16, False), _case(1, 96, 192, R.SILU, R.F16, False),
         _case(4, 200, 8256, R.PLAIN, R.F32, False), _case(4, 96, 8256, R.SILU, R.F16, False),
         _case(1, 200, 192, R.PLAIN, R.F16, True), _case(1, 96, 192, R.SILU, R.F16, True),
         _case(4, 200, 8256, R.PLAIN, R.F32, True), _case(4, 96, 8256, R.SILU, R.F16, True), _case(2, 1000, 4096, R.PLAIN, R.F32, True),
         # the stream kernel: one panel x the whole K; 4 and 5 panels x 4 k-parts combined inside the launch (fragment-ordered A)
         _case(5, 3072, 1024, R.PLAIN, R.F16, False), _case(37, 3072, 1024, R.GELU, R.F16, False),
         _case(27, 3072, 14336, R.PLAIN, R.F32, False, True), _case(20, 4160, 2048, R.GELU, R.F16, False, True),
         # the mid kernel: one k-part, k-parts through the reduce, the fused norm with the gate / up pair, the 4-tile form
         _case(5, 200, 192, R.PLAIN, R.F16, False), _case(5, 200, 512, R.GELU, R.F16, False), _case(5, 96, 512, R.SILU, R.F16, True),
         _case(37, 1280, 512, R.PLAIN, R.F32, True),
         # the wide kernel: 2 / 4 / 6 row tiles, one k-part and k-parts through the reduce, the gate / up pair
         _case(5, 16392, 192, R.PLAIN, R.F16, False), _case(37, 16384, 1024, R.SILU, R.F16, False), _case(20, 16384, 512, R.GELU, R.F16, False),
         _case(70, 16384, 1024, R.PLAIN, R.F32, False)]


@pytest.mark.parametrize("c", GAUSS, ids=R.case_id)
def test_w8_gaussian_operands_with_spread_row_exponents(ctx, dev, c):
    obs = Q.run_gaussian_case(ctx, dev, c)
    print("w8_gauss", obs)
    record("w8_gauss." + obs["id"], {k: obs[k] for k in ("err", "ref_max", "dq_rel_rms", "exp_spread_in_panel")})
    assert obs["exp_spread_in_panel"] >= 6 and obs.get("exp_spread_in_pair", 6) >= 6
    assert obs["ran_w8"] == [1] and obs["plans"] == [list(c.plan)]
    assert obs["finite"] and obs["guard_untouched"]
    assert obs["err"] <= K.bound(c, obs), (obs["err"], K.bound(c, obs))


# ------------------------------------------------------------------------------------------------ 5. model level
def _pair(cfg, dev, seed=0):
    """(FP8 model, its twin on the same dequantised weights without FP8 tensors)"""
    m8 = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, seed, dev, decoder_weights="fp8"), dev)
    m16 = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, seed, dev, decoder_weights="fp8_dequantized"), dev)
    return m8, m16


def _ragged(cfg, B):
    lens = [(14, 5), (9, 2), (11, 3), (7, 1)]
    rows = [synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=lens[i % 4][0], seq_pos=lens[i % 4][1]) for i in range(B)]
    width = max(len(r) for r in rows)
    ids = torch.full((B, width), 2, dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, width - len(r):] = torch.tensor(r)                 # left-padded
    return ids, ids != 2, [synth.synth_protein(20 + 7 * i, i) for i in range(B)]


def _embed(model, ids, mask, seqs):
    prot = model.switch_projector_embedding(model.encode_projector_embedding(model.encode_seq2embedding(seqs)))
    emb, mo, _ = model._splice(ids, mask, prot, True)
    return emb, mo


def _margin(lg):
    t = lg.float().topk(2, dim=-1).values
    return t[:, 0] - t[:, 1]


def _compare_steps(m8, m16, emb, mask, steps, tag, per_step_w8):
    """prefill bit-identical (prefill reads the fp16 tensors of either model); `steps` decode steps forced with the twin's greedy
    ids: logits within DECODE_BOUND, ids equal wherever the twin's margin exceeds MARGIN_TAU; the FP8 model's GEMM count."""
    lg8, lg16 = m8.prefill_logits(emb, mask), m16.prefill_logits(emb, mask)
    assert torch.equal(lg8, lg16)
    assert m8.stat("w8_gemms") == 0
    worst, decisive, total, identical = 0.0, 0, 0, True
    tok = lg16.argmax(-1)
    for s in range(steps):
        a, b = m8.decode_logits(tok), m16.decode_logits(tok)
        assert torch.isfinite(a).all()
        worst = max(worst, rel_l2(a, b))
        identical = identical and torch.equal(a, b)
        dec = _margin(b) > MARGIN_TAU
        assert torch.equal(a.argmax(-1)[dec], b.argmax(-1)[dec]), (tag, s)
        decisive, total = decisive + int(dec.sum()), total + dec.numel()
        tok = b.argmax(-1)
    print("w8_model", tag, "rel_l2", worst, "bit_identical", identical, "decisive", decisive, "of", total)
    record("w8_model." + tag, {"rel_l2": worst, "bit_identical": identical, "decisive": decisive, "steps": total})
    assert worst <= DECODE_BOUND, (tag, worst)
    assert 4 * decisive >= 3 * total, (tag, decisive, total)
    assert m8.stat("w8_gemms") == per_step_w8 * steps and m16.stat("w8_gemms") == 0
    return worst


@pytest.mark.parametrize("preset", ["micro", "micro_qwen"])
def test_fp8_micro_model_against_its_dequantised_twin(dev, preset):
    cfg = opa.PRESETS[preset]()
    m8, m16 = _pair(cfg, dev)
    assert m8.decoder_weight_format == "fp8" and m16.decoder_weight_format == "fp8_dequantized"
    assert OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev).decoder_weight_format == ("bf16" if _cabi.BF16 else "fp16")
    names = [n for n in m8.weights.tensors if n.endswith(".q8")]
    assert len(names) == 4 * cfg.dec_layers and not [n for n in m16.weights.tensors if n.endswith((".q8", ".e8"))]
    for n in names:                                               # the fp16 tensors ARE the dequantised codes, and the twin's too
        q, e = untile_fp8(m8.weights.tensors[n]).cpu(), m8.weights.tensors[n[:-3] + ".e8"].cpu()
        dq = W8.e4m3_values()[q.long()] * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())[:, None]
        assert torch.equal(untile_weight(m8.weights.tensors[n[:-3]]).cpu().double(), dq)
        assert torch.equal(m8.weights.tensors[n[:-3]], m16.weights.tensors[n[:-3]])
    assert m8.weights.nbytes() > m16.weights.nbytes()
    ids, mask, seqs = _ragged(cfg, 3)
    emb, mo = _embed(m16, ids, mask, seqs)
    _compare_steps(m8, m16, emb, mo, 6, preset + ".b3", 4 * cfg.dec_layers)
    m8b = m8.new_context()                                        # shares the tensors, FP8 ones included
    assert m8b.weights is m8.weights and m8b.decoder_weight_format == "fp8"
    m8b.prefill_logits(emb, mo)
    m8b.decode_logits(torch.zeros(3, dtype=torch.int32))
    assert m8b.stat("w8_gemms") == 4 * cfg.dec_layers


def test_fp8_from_canonical_is_the_synthetic_fill(dev):
    cfg = opa.micro()
    a = DeviceWeights.from_canonical(cfg, synth.canonical_weights(cfg, 0), dev, decoder_weights="fp8")
    b = DeviceWeights.synthetic(cfg, 0, dev, decoder_weights="fp8")
    assert sorted(a.tensors) == sorted(b.tensors)
    for n in a.tensors:
        if n.startswith("dec.") and n.endswith((".q8", ".e8")):
            assert torch.equal(a.tensors[n], b.tensors[n]), n
    with pytest.raises(ValueError):
        DeviceWeights.synthetic(cfg, 0, dev, decoder_weights="nf4")


@pytest.mark.parametrize("B", [1, 4, 5, 16, 17, 64])
def test_fp8_llama3_8b_widths(dev, wide_pair, B):
    """Llama-3-8B widths x 2 decoder layers, three decode steps: every layer GEMM streams the FP8 panels (1 .. 4 rows: the skinny
    kernel; 5 .. 64 rows: the stream kernel for QKV, wo and down, the wide kernel with the row scale for gate / up)."""
    cfg, m8, m16 = wide_pair
    g = torch.Generator().manual_seed(B)
    T = 24
    emb = (torch.randn(B, T, cfg.dec_dim, generator=g) * 0.05).to(_cabi.operand_dtype())
    mask = torch.ones(B, T, dtype=torch.bool)
    for b in range(B):
        mask[b, :(3 * b) % 7] = False                            # ragged, left-padded
    before = m8.stat("w8_gemms")
    m8.prefill_logits(emb, mask)
    assert m8.stat("w8_gemms") == before
    lg16 = m16.prefill_logits(emb, mask)
    tok, worst = lg16.argmax(-1), 0.0
    for s in range(3):
        a, b_ = m8.decode_logits(tok), m16.decode_logits(tok)
        worst = max(worst, rel_l2(a, b_))
        tok = b_.argmax(-1)
    print("w8_model wide B", B, "rel_l2", worst)
    record(f"w8_model.llama3_8b_widths.b{B}", worst)
    assert worst <= DECODE_BOUND
    assert m8.stat("w8_gemms") - before == 3 * 4 * cfg.dec_layers


@pytest.fixture(scope="module")
def wide_pair(dev):
    cfg = opa.OpusConfig(enc_layers=1, enc_dim=64, enc_heads=4, enc_ffn=128, proj_dim=64, switch_depth=1, n_prot_tokens=1,
                         dec_layers=2, dec_dim=4096, dec_heads=32, dec_kv_heads=8, dec_head_dim=128, dec_ffn=14336,
                         dec_vocab=32768, dec_rope_theta=500000.0, max_batch=64, max_enc_tokens=34, max_prompt=32,
                         max_new_tokens=8).validate()
    m8, m16 = _pair(cfg, dev)
    yield cfg, m8, m16
    del m8, m16
    torch.cuda.empty_cache()


def test_fp8_opt_model_runs_on_the_dequantised_tensors(dev):
    cfg = opa.micro_opt()
    m8, m16 = _pair(cfg, dev)
    assert m8.decoder_weight_format == "fp8" and not [n for n in m8.weights.tensors if n.endswith(".q8")]
    ids, mask, seqs = _ragged(cfg, 3)
    kw = dict(attention_mask=mask, pad_token_id=2, do_sample=False, max_new_tokens=8)
    assert torch.equal(m8.generate(ids, seqs, **kw), m16.generate(ids, seqs, **kw))
    plain = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    assert not torch.equal(m8.weights.tensors["dec.0.w1"], plain.weights.tensors["dec.0.w1"])      # quantised all the same


def test_fp8_generate_graph_replay_sampling_and_trie(dev):
    cfg = opa.micro()
    m8, m16 = _pair(cfg, dev)
    ids, mask, seqs = _ragged(cfg, 3)
    kw = dict(attention_mask=mask, pad_token_id=2, max_new_tokens=8)
    a, b = m8.generate(ids, seqs, do_sample=False, **kw), m8.generate(ids, seqs, do_sample=False, **kw)
    assert torch.equal(a, b) and m8.stat("graph_replays") > 0                      # the captured step, replayed
    assert m8.stat("w8_gemms") >= 4 * cfg.dec_layers
    ref = m16.generate(ids, seqs, do_sample=False, **kw)
    # The FP8 kernels multiply the same numbers in the same order and scale the fp32 sums by a power of two: the decode logits are
    # the twin's bit for bit (asserted at 3 rows, the skinny kernel), so every step is decisive - greedy ids, the draws of the 6-row
    # sampling run (mid kernels at these widths) and the constrained ids agree.
    emb, mo = _embed(m16, ids, mask, seqs)
    assert torch.equal(m8.prefill_logits(emb, mo), m16.prefill_logits(emb, mo))
    for s in range(8):
        assert torch.equal(m8.decode_logits(ref[:, s]), m16.decode_logits(ref[:, s])), s
    assert torch.equal(a, ref)
    samp = dict(do_sample=True, temperature=0.8, top_p=0.9, seed=5, num_return_sequences=2)
    s8, s16 = m8.generate(ids, seqs, **samp, **kw), m16.generate(ids, seqs, **samp, **kw)
    assert s8.shape == (6, 8) and torch.equal(s8, s16)
    trie = TokenTrie([[5, 6, 7], [5, 9], [11, 12, 13, 14], [20]], end_token_id=3)
    t8 = m8.generate(ids, seqs, do_sample=False, eos_token_id=3, prefix_allowed_tokens_fn=trie, **kw)
    t16 = m16.generate(ids, seqs, do_sample=False, eos_token_id=3, prefix_allowed_tokens_fn=trie, **kw)
    assert torch.equal(t8, t16) and t8.shape[1] >= 2              # (ran to completion: a member and the end id)


# ------------------------------------------------------------------------------------------------ 7. quality drift (measured)
def test_fp8_drift_against_the_unquantised_model_is_recorded(dev):
    """The mid-size model of tests/test_gpu_parity.py: FP8 model against the UNQUANTISED model (another model: e4m3 keeps 4
    significant bits, ~2.6 % relative rms per weight) over prefill + 8 forced decode steps.  Measured and recorded, not bounded:
    the figures are in DESIGN.md section 3 and profiles/w8_parity.jsonl."""
    cfg = opa.OpusConfig(enc_layers=2, enc_dim=1280, enc_heads=20, enc_ffn=5120, proj_dim=1024,
                         dec_layers=2, dec_dim=1024, dec_heads=8, dec_kv_heads=2, dec_head_dim=128, dec_ffn=2816,
                         dec_vocab=4096, max_batch=4, max_enc_tokens=300, max_prompt=64, max_new_tokens=16).validate()
    m8 = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev, decoder_weights="fp8"), dev)
    m16 = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    ids, mask, _ = _ragged(cfg, 3)
    seqs = [synth.synth_protein(n, i) for i, n in enumerate((200, 77, 131))]
    emb, mo = _embed(m16, ids, mask, seqs)
    a, b = m8.prefill_logits(emb, mo), m16.prefill_logits(emb, mo)
    rels, agree, total = [rel_l2(a, b)], int((a.argmax(-1) == b.argmax(-1)).sum()), 3
    tok = b.argmax(-1)
    for s in range(8):
        a, b = m8.decode_logits(tok), m16.decode_logits(tok)
        assert torch.isfinite(a).all()
        rels.append(rel_l2(a, b))
        agree, total = agree + int((a.argmax(-1) == b.argmax(-1)).sum()), total + 3
        tok = b.argmax(-1)
    print("w8_drift rel_l2 max", max(rels), "mean", sum(rels) / len(rels), "greedy ids agreeing", agree, "of", total)
    record("w8_drift.midsize", {"rel_l2_max": max(rels), "rel_l2_mean": sum(rels) / len(rels), "ids_agree": agree, "ids": total})


# ------------------------------------------------------------------------------------------------ 6. the bf16 build
def test_bf16_build_w8():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_w8_check.py")], capture_output=True, text=True,
                       env=dict(os.environ, OPUS_DTYPE="bf16"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_W8 ")][-1]
    o = json.loads(line[len("BF16_W8 "):])
    assert o["operand_dtype"] == 1 and o["quantiser_is_twin"], o
    cases = {R.case_id(c): c for c in R.bf16_subset() if c.plan.klass in Q.W8_CLASSES}
    assert sorted(o["cases"]) == sorted(cases) and cases
    bad = {n: Q.failures(cases[n], x, bf16=True) for n, x in o["cases"].items()}
    bad = {n: b for n, b in bad.items() if b}
    assert not bad, bad
    record("w8_model.bf16.micro", o["micro"])
    assert o["micro"]["prefill_identical"] and o["micro"]["rel_l2"] <= R.BF16_FACTOR * DECODE_BOUND and o["micro"]["w8_gemms"] == 6 * 8
