"""MXFP4 decoder weights on the GPU: the load-time quantiser against its CPU twin (bit for bit), every GEMM cell of the skinny, mid,
wide and stream kernels with the MXFP4 form of W (route unchanged, MXFP4 panels streamed, exact result on operands that put every
code under eight scale bytes - the check of v_cvt_scalef32_pk_{f16,bf16}_fp4), the fall-back of the classes without an MXFP4 form
(ring, tile, pp), Gaussian operands, and the MXFP4 model against the model of the same dequantised weights without MXFP4 tensors
(decoder_weights="mxfp4_dequantized").

Observed figures of a run: profiles/w4_parity.jsonl.
"""
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
from opus_pllm_amd.weights import DeviceWeights, quantize_mxfp4, untile_mxfp4, untile_weight
import gemm_cells_checks as K
import gemm_cells_ref as R
import w4_checks as Q4
import w4_ref as W4
from gpu_helpers import record, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_TAU = 0.05
DECODE_BOUND = 2e-3                # tests/test_gpu_batch64.py: decode step vs prefill of the longer prompt
# The weights seed of the model pairs.  The cap "3/4 of the (row, step) pairs are decisive" is a condition on the TWIN's margins
# (existing kernels only): seed 0 meets it on every pair below (the figures are in profiles/w4_parity.jsonl).
SEED = 0


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
    edge = W4.edge_rows(Kk, dt)
    n = min(len(edge), N)
    W[:n] = edge[:n]                                              # the rules' edges, planted
    return W


def _check_quantiser(W, dev):
    q_ref, s_ref, dq_ref = W4.quantize(W)
    q4, s4, dq = quantize_mxfp4(W.to(dev))
    torch.cuda.synchronize()
    codes, scales = untile_mxfp4(q4, s4)
    assert torch.equal(scales.cpu(), s_ref)
    assert torch.equal(codes.cpu(), q_ref)
    assert torch.equal(q4.cpu(), W4.tile(q_ref)) and torch.equal(s4.cpu(), W4.tile_scales(s_ref))
    assert torch.equal(K._bits(dq.cpu()), K._bits(dq_ref))
    assert 1 <= int(s4.min()) and int(s4.max()) <= 254 and not (codes == 8).any()


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
    e = W4.block_exponents(W.to(dt)).view(2, 2, 16, 4)
    assert int((e[:, 0].float().mean() - e[:, 1].float().mean()).abs()) >= 5


def test_quantiser_in_place_and_refusals(dev):
    dt = _cabi.operand_dtype()
    W = _weights(32, 128, dt, 9).to(dev)
    q4, s4, dq = quantize_mxfp4(W)
    q2, s2 = torch.empty_like(q4), torch.empty_like(s4)
    W2 = W.clone()
    _cabi.check(_cabi.lib().opus_quantize_mxfp4(W2.data_ptr(), 32, 128, q2.data_ptr(), s2.data_ptr(), W2.data_ptr(), None))   # dq over src
    assert torch.equal(K._bits(W2), K._bits(dq)) and torch.equal(q2, q4) and torch.equal(s2, s4)
    for bad in (float("nan"), float("inf"), -float("inf")):
        Wb = W.clone()
        Wb[17, 77] = bad
        with pytest.raises(_cabi.OpusError, match="not finite"):
            quantize_mxfp4(Wb)
    lib = _cabi.lib()
    assert lib.opus_quantize_mxfp4(W.data_ptr(), 24, 128, q2.data_ptr(), s2.data_ptr(), None, None) == -2      # N % 16
    assert lib.opus_quantize_mxfp4(W.data_ptr(), 32, 96, q2.data_ptr(), s2.data_ptr(), None, None) == -2       # K % 64
    assert lib.opus_quantize_mxfp4(None, 32, 128, q2.data_ptr(), s2.data_ptr(), None, None) == -1


# ------------------------------------------------------------------------------------------------ 3. cells
ALL = R.CASES + R.SLAB_CASES
W4_CASES = [c for c in ALL if R.route_case(c) is not None and R.route_case(c).klass in Q4.W4_CLASSES]


def _first(klass):
    return next(c for c in ALL if c.plan.klass == klass and c.M * c.N * c.K < 1 << 28)


# one case of every class without an MXFP4 form: the launch reads the 16-bit copy
FALLBACK_CASES = [_first(k) for k in (R.RING, R.TILE)] + [next(c for c in ALL if c.plan.klass == R.PP)]


def test_case_tables():
    assert len(W4_CASES) >= 150 and all(c.plan.klass in Q4.W4_CLASSES for c in W4_CASES)
    assert len(W4_CASES) == len([c for c in ALL if c.plan.klass in (R.SKINNY, R.MID, R.WIDE, R.STREAM)])
    cells = {R.cell_of(c) for c in W4_CASES}
    assert cells == {c for c in R.CELLS + R.SLAB_CELLS if c.klass in Q4.W4_CLASSES}
    assert all(c.plan.klass not in Q4.W4_CLASSES for c in FALLBACK_CASES)


@pytest.mark.parametrize("c", W4_CASES, ids=R.case_id)
def test_w4_cell_routes_as_before_and_is_exact(ctx, dev, c):
    assert R.route_case(c) == c.plan
    obs = Q4.run_exact_case(ctx, dev, c, repeats=K.REPEATS if c.plan.combine == R.IN_LAUNCH else 2)
    if "exact" not in obs:
        print("w4_cells", obs["id"], "err", obs["err"], "ref_max", obs["ref_max"], "bound", K.bound(c, obs))
        record("w4_cells." + obs["id"], {"err": obs["err"], "ref_max": obs["ref_max"], "bound": K.bound(c, obs)})
    bad = Q4.failures(c, obs)
    assert not bad, (obs["id"], bad)


@pytest.mark.parametrize("c", FALLBACK_CASES, ids=R.case_id)
def test_class_without_mxfp4_form_reads_the_16_bit_copy(ctx, dev, c):
    obs = Q4.run_exact_case(ctx, dev, c)
    assert obs["ran_w4"] == [0]
    bad = Q4.failures(c, obs)
    assert not bad, (obs["id"], bad)


# ------------------------------------------------------------------------------------------------ 4. Gaussian operands
def _case(M, N, Kk, epi, mode, norm, a_tiled=False):
    return next(c for c in R.CASES if (c.M, c.N, c.K, c.epi, c.mode, c.norm, c.a_tiled) == (M, N, Kk, epi, mode, norm, a_tiled))


# (the GAUSS list of tests/test_gpu_w8.py)
GAUSS = [_case(1, 200, 192, R.PLAIN, R.F16, False), _case(1, 200, 192, R.GELU, R.F16, False), _case(1, 96, 192, R.SILU, R.F16, False),
         _case(4, 200, 8256, R.PLAIN, R.F32, False), _case(4, 96, 8256, R.SILU, R.F16, False),
         _case(1, 200, 192, R.PLAIN, R.F16, True), _case(1, 96, 192, R.SILU, R.F16, True),
         _case(4, 200, 8256, R.PLAIN, R.F32, True), _case(4, 96, 8256, R.SILU, R.F16, True), _case(2, 1000, 4096, R.PLAIN, R.F32, True),
         _case(5, 3072, 1024, R.PLAIN, R.F16, False), _case(37, 3072, 1024, R.GELU, R.F16, False),
         _case(27, 3072, 14336, R.PLAIN, R.F32, False, True), _case(20, 4160, 2048, R.GELU, R.F16, False, True),
         _case(5, 200, 192, R.PLAIN, R.F16, False), _case(5, 200, 512, R.GELU, R.F16, False), _case(5, 96, 512, R.SILU, R.F16, True),
         _case(37, 1280, 512, R.PLAIN, R.F32, True),
         _case(5, 16392, 192, R.PLAIN, R.F16, False), _case(37, 16384, 1024, R.SILU, R.F16, False), _case(20, 16384, 512, R.GELU, R.F16, False),
         _case(70, 16384, 1024, R.PLAIN, R.F32, False)]


@pytest.mark.parametrize("c", GAUSS, ids=R.case_id)
def test_w4_gaussian_operands_with_spread_scales(ctx, dev, c):
    obs = Q4.run_gaussian_case(ctx, dev, c)
    print("w4_gauss", obs)
    record("w4_gauss." + obs["id"], {k: obs[k] for k in ("err", "ref_max", "dq_rel_rms", "scale_spread_in_panel", "scale_spread_along_k")})
    assert obs["scale_spread_in_panel"] >= 6 and obs.get("scale_spread_in_pair", 6) >= 6
    assert obs["ran_w4"] == [1] and obs["plans"] == [list(c.plan)]
    assert obs["finite"] and obs["guard_untouched"]
    assert obs["err"] <= K.bound(c, obs), (obs["err"], K.bound(c, obs))


# ------------------------------------------------------------------------------------------------ 5. model level
def _pair(cfg, dev, seed=SEED):
    """(MXFP4 model, its twin on the same dequantised weights without MXFP4 tensors)"""
    m4 = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, seed, dev, decoder_weights="mxfp4"), dev)
    m16 = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, seed, dev, decoder_weights="mxfp4_dequantized"), dev)
    return m4, m16


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


def _compare_steps(m4, m16, emb, mask, steps, tag, per_step_w4):
    """prefill bit-identical (prefill reads the 16-bit tensors of either model); `steps` decode steps forced with the twin's greedy
    ids: logits within DECODE_BOUND, ids equal wherever the twin's margin exceeds MARGIN_TAU; the MXFP4 model's GEMM count."""
    before = m4.stat("w4_gemms")
    lg4, lg16 = m4.prefill_logits(emb, mask), m16.prefill_logits(emb, mask)
    assert torch.equal(lg4, lg16)
    assert m4.stat("w4_gemms") == before
    worst, decisive, total, identical = 0.0, 0, 0, True
    tok = lg16.argmax(-1)
    for s in range(steps):
        a, b = m4.decode_logits(tok), m16.decode_logits(tok)
        assert torch.isfinite(a).all()
        worst = max(worst, rel_l2(a, b))
        identical = identical and torch.equal(a, b)
        dec = _margin(b) > MARGIN_TAU
        assert torch.equal(a.argmax(-1)[dec], b.argmax(-1)[dec]), (tag, s)
        decisive, total = decisive + int(dec.sum()), total + dec.numel()
        tok = b.argmax(-1)
    print("w4_model", tag, "rel_l2", worst, "bit_identical", identical, "decisive", decisive, "of", total)
    record("w4_model." + tag, {"rel_l2": worst, "bit_identical": identical, "decisive": decisive, "steps": total})
    assert worst <= DECODE_BOUND, (tag, worst)
    assert 4 * decisive >= 3 * total, (tag, decisive, total)
    assert m4.stat("w4_gemms") - before == per_step_w4 * steps and m16.stat("w4_gemms") == 0 and m4.stat("w8_gemms") == 0
    return worst


@pytest.mark.parametrize("preset", ["micro", "micro_qwen"])
def test_mxfp4_micro_model_against_its_dequantised_twin(dev, preset):
    cfg = opa.PRESETS[preset]()
    m4, m16 = _pair(cfg, dev)
    assert m4.decoder_weight_format == "mxfp4" and m16.decoder_weight_format == "mxfp4_dequantized"
    names = [n for n in m4.weights.tensors if n.endswith(".q4")]
    assert len(names) == 4 * cfg.dec_layers and not [n for n in m16.weights.tensors if n.endswith((".q4", ".s4", ".q8", ".e8"))]
    for n in names:                                               # the 16-bit tensors ARE the dequantised codes, and the twin's too
        q, s = untile_mxfp4(m4.weights.tensors[n], m4.weights.tensors[n[:-3] + ".s4"])
        assert torch.equal(untile_weight(m4.weights.tensors[n[:-3]]).cpu().double(), W4.dequantize(q.cpu(), s.cpu()))
        assert torch.equal(m4.weights.tensors[n[:-3]], m16.weights.tensors[n[:-3]])
        t16 = m4.weights.tensors[n[:-3]]
        assert m4.weights.tensors[n].numel() + m4.weights.tensors[n[:-3] + ".s4"].numel() <= 0.27 * 2 * t16.numel()
    assert m4.weights.nbytes() > m16.weights.nbytes()
    ids, mask, seqs = _ragged(cfg, 3)
    emb, mo = _embed(m16, ids, mask, seqs)
    _compare_steps(m4, m16, emb, mo, 6, preset + ".b3", 4 * cfg.dec_layers)
    m4b = m4.new_context()                                        # shares the tensors, MXFP4 ones included
    assert m4b.weights is m4.weights and m4b.decoder_weight_format == "mxfp4"
    m4b.prefill_logits(emb, mo)
    m4b.decode_logits(torch.zeros(3, dtype=torch.int32))
    assert m4b.stat("w4_gemms") == 4 * cfg.dec_layers


def test_mxfp4_from_canonical_is_the_synthetic_fill(dev):
    cfg = opa.micro()
    a = DeviceWeights.from_canonical(cfg, synth.canonical_weights(cfg, 0), dev, decoder_weights="mxfp4")
    b = DeviceWeights.synthetic(cfg, 0, dev, decoder_weights="mxfp4")
    assert sorted(a.tensors) == sorted(b.tensors)
    for n in a.tensors:
        if n.startswith("dec.") and n.endswith((".q4", ".s4")):
            assert torch.equal(a.tensors[n], b.tensors[n]), n
    with pytest.raises(ValueError):
        DeviceWeights.synthetic(cfg, 0, dev, decoder_weights="nf4")


@pytest.fixture(scope="module")
def wide_pair(dev):
    cfg = opa.OpusConfig(enc_layers=1, enc_dim=64, enc_heads=4, enc_ffn=128, proj_dim=64, switch_depth=1, n_prot_tokens=1,
                         dec_layers=2, dec_dim=4096, dec_heads=32, dec_kv_heads=8, dec_head_dim=128, dec_ffn=14336,
                         dec_vocab=32768, dec_rope_theta=500000.0, max_batch=64, max_enc_tokens=34, max_prompt=32,
                         max_new_tokens=8).validate()
    m4, m16 = _pair(cfg, dev)
    yield cfg, m4, m16
    del m4, m16
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [1, 4, 5, 16, 17, 64])
def test_mxfp4_llama3_8b_widths(dev, wide_pair, B):
    """Llama-3-8B widths x 2 decoder layers, three decode steps: every layer GEMM streams the MXFP4 panels (1 .. 4 rows: the skinny
    kernel; 5 .. 64 rows: the stream kernel for QKV, wo and down, the wide kernel with the row scale for gate / up)."""
    cfg, m4, m16 = wide_pair
    g = torch.Generator().manual_seed(B)
    emb = (torch.randn(B, 24, cfg.dec_dim, generator=g) * 0.05).to(_cabi.operand_dtype())
    mask = torch.ones(B, 24, dtype=torch.bool)
    for b in range(B):
        mask[b, :(3 * b) % 7] = False                            # ragged, left-padded
    _compare_steps(m4, m16, emb, mask, 3, f"llama3_8b_widths.b{B}", 4 * cfg.dec_layers)


def test_mxfp4_opt_model_runs_on_the_dequantised_tensors(dev):
    cfg = opa.micro_opt()
    m4, m16 = _pair(cfg, dev)
    assert m4.decoder_weight_format == "mxfp4" and not [n for n in m4.weights.tensors if n.endswith((".q4", ".s4"))]
    ids, mask, seqs = _ragged(cfg, 3)
    kw = dict(attention_mask=mask, pad_token_id=2, do_sample=False, max_new_tokens=8)
    assert torch.equal(m4.generate(ids, seqs, **kw), m16.generate(ids, seqs, **kw))
    assert m4.stat("w4_gemms") == 0
    plain = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    assert not torch.equal(m4.weights.tensors["dec.0.w1"], plain.weights.tensors["dec.0.w1"])      # quantised all the same


def test_mxfp4_generate_graph_replay_sampling_trie_and_lookup(dev):
    cfg = opa.micro(max_batch=24)                                 # (a lookup pass verifies batch x (k + 1) = 3 x 8 positions)
    m4, m16 = _pair(cfg, dev)
    ids, mask, seqs = _ragged(cfg, 3)
    kw = dict(attention_mask=mask, pad_token_id=2, max_new_tokens=8)
    a, b = m4.generate(ids, seqs, do_sample=False, **kw), m4.generate(ids, seqs, do_sample=False, **kw)
    assert torch.equal(a, b) and m4.stat("graph_replays") > 0                      # the captured step, replayed
    assert m4.stat("w4_gemms") >= 4 * cfg.dec_layers
    ref = m16.generate(ids, seqs, do_sample=False, **kw)
    # The MXFP4 kernels feed the MFMAs the twin's operands in the twin's order: the decode logits are expected to be the twin's bit
    # for bit (asserted here at 3 rows), so every step is decisive - greedy ids, the draws of the 6-row sampling run, the
    # constrained ids and the prompt-lookup ids agree.
    emb, mo = _embed(m16, ids, mask, seqs)
    assert torch.equal(m4.prefill_logits(emb, mo), m16.prefill_logits(emb, mo))
    for s in range(8):
        assert torch.equal(m4.decode_logits(ref[:, s]), m16.decode_logits(ref[:, s])), s
    assert torch.equal(a, ref)
    samp = dict(do_sample=True, temperature=0.8, top_p=0.9, seed=5, num_return_sequences=2)
    s4, s16 = m4.generate(ids, seqs, **samp, **kw), m16.generate(ids, seqs, **samp, **kw)
    assert s4.shape == (6, 8) and torch.equal(s4, s16)
    trie = TokenTrie([[5, 6, 7], [5, 9], [11, 12, 13, 14], [20]], end_token_id=3)
    t4 = m4.generate(ids, seqs, do_sample=False, eos_token_id=3, prefix_allowed_tokens_fn=trie, **kw)
    t16 = m16.generate(ids, seqs, do_sample=False, eos_token_id=3, prefix_allowed_tokens_fn=trie, **kw)
    assert torch.equal(t4, t16) and t4.shape[1] >= 2              # (ran to completion: a member and the end id)
    # prompt lookup: drafts taken from the twin's own answer, so that verify passes run - on the MXFP4 panels
    lk = dict(do_sample=False, prompt_lookup_num_tokens=7, lookup_ids=ref, **kw)
    before, passes = m4.stat("w4_gemms"), m4.stat("lookup_passes")
    assert torch.equal(m4.generate(ids, seqs, **lk), m16.generate(ids, seqs, **lk))
    assert m4.stat("w4_gemms") > before and m4.stat("lookup_passes") > passes and m16.stat("w4_gemms") == 0


# ------------------------------------------------------------------------------------------------ 7. quality drift (measured)
def test_mxfp4_drift_against_the_unquantised_model_is_recorded(dev):
    """The mid-size model of tests/test_gpu_parity.py: MXFP4 model against the UNQUANTISED model (another model: e2m1 keeps 2
    significant bits, ~11 % relative rms per row) over prefill + 8 forced decode steps.  Measured and recorded, not bounded: the
    figures are in DESIGN.md section 3 and profiles/w4_parity.jsonl."""
    cfg = opa.OpusConfig(enc_layers=2, enc_dim=1280, enc_heads=20, enc_ffn=5120, proj_dim=1024,
                         dec_layers=2, dec_dim=1024, dec_heads=8, dec_kv_heads=2, dec_head_dim=128, dec_ffn=2816,
                         dec_vocab=4096, max_batch=4, max_enc_tokens=300, max_prompt=64, max_new_tokens=16).validate()
    m4 = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev, decoder_weights="mxfp4"), dev)
    m16 = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    ids, mask, _ = _ragged(cfg, 3)
    seqs = [synth.synth_protein(n, i) for i, n in enumerate((200, 77, 131))]
    emb, mo = _embed(m16, ids, mask, seqs)
    a, b = m4.prefill_logits(emb, mo), m16.prefill_logits(emb, mo)
    rels, agree, total, margins = [rel_l2(a, b)], int((a.argmax(-1) == b.argmax(-1)).sum()), 3, _margin(b).tolist()
    tok = b.argmax(-1)
    for s in range(8):
        a, b = m4.decode_logits(tok), m16.decode_logits(tok)
        assert torch.isfinite(a).all()
        rels.append(rel_l2(a, b))
        agree, total = agree + int((a.argmax(-1) == b.argmax(-1)).sum()), total + 3
        margins += _margin(b).tolist()
        tok = b.argmax(-1)
    margins.sort()
    fig = {"rel_l2_max": max(rels), "rel_l2_mean": sum(rels) / len(rels), "ids_agree": agree, "ids": total,
           "margin_min": margins[0], "margin_median": margins[len(margins) // 2], "margin_max": margins[-1]}
    print("w4_drift", fig)
    record("w4_drift.midsize", fig)


# ------------------------------------------------------------------------------------------------ 6. the bf16 build
def test_bf16_build_w4():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_w4_check.py")], capture_output=True, text=True,
                       env=dict(os.environ, OPUS_DTYPE="bf16"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_W4 ")][-1]
    o = json.loads(line[len("BF16_W4 "):])
    assert o["operand_dtype"] == 1 and o["quantiser_is_twin"], o
    # one cell per class: of gemm_cells_ref.bf16_subset(), per class the case whose k-parts take the longest way
    cases = {R.case_id(c): c for c in bf16_cells()}
    assert sorted(o["cases"]) == sorted(cases) and len(cases) == 4
    bad = {n: Q4.failures(cases[n], x, bf16=True) for n, x in o["cases"].items()}
    bad = {n: b for n, b in bad.items() if b}
    assert not bad, bad
    record("w4_model.bf16.micro", o["micro"])
    assert o["micro"]["prefill_identical"] and o["micro"]["rel_l2"] <= R.BF16_FACTOR * DECODE_BOUND and o["micro"]["w4_gemms"] == 6 * 8


def bf16_cells():
    best = {}
    for c in R.bf16_subset():
        k = c.plan.klass
        if k in Q4.W4_CLASSES and (k not in best or c.plan.combine > best[k].plan.combine):
            best[k] = c
    return list(best.values())
