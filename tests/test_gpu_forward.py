"""OpusLlamaForCausalLM.forward(labels=...) on the GPU: teacher-forced loss, token log-probs and logits (the reference's forward,
opus_llama.py:41-92), the NLL kernel alone (opus_debug_xent), the three decoder families, batches above max_batch, padding and
what the call leaves in the context.  The bf16 build runs the same checks in a child process (tests/bf16_forward_check.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
import forward_checks as fc
from gpu_helpers import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REL_L2 = 1.5e-2            # logits at valid positions vs the reference / oracle (fp16 operands)
LOSS_REL_GOLD = 2e-3       # loss vs the reference's forward (micro)
LP_ABS_GOLD = 2e-2         # token log-probs vs the reference's logits (fp64 log_softmax)
XENT_ABS = 1e-4            # NLL kernel vs fp64
LP_ABS_ORACLE = 2e-2       # token log-probs vs the fp32 oracle
LOSS_REL_ORACLE = 1e-2
PATHS_ABS = 1e-3           # loss-only path vs return_logits path ...
# ... or 2 units in the last place of the largest logit, whichever is larger: the two paths run the lm_head over different row
# counts (other GEMM kernels, fused or separate norm), and each rounds its logits to the operand dtype as the model's lm_head does
# (fp16 / bf16 spacing at |l|: 2^-10 / 2^-7 of it) - the synthetic micro models have logits of tens
ULP_REL = 2.0 ** -10
ROW_ALONE_ABS = 1.5e-2     # a row scored alone vs its row of the batch (token log-probs)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def test_golden_cases_match_reference_forward(dev):
    obs = fc.golden_cases(dev)
    record("forward.golden", obs)
    for tag, o in obs.items():
        assert o["shape_ok"], (tag, o)
        assert o["logits_rel_l2"] < REL_L2, (tag, o)
        assert o["argmax_bad"] == 0 and o["argmax_checked"] > 0, (tag, o)
        if tag == "d":
            assert o["loss_is_none"], o
        else:
            assert o["loss_rel"] < LOSS_REL_GOLD and o["lp_abs"] < LP_ABS_GOLD and o["n_tokens_ok"], (tag, o)


def test_xent_kernel_vs_fp64(dev):
    o = fc.xent_kernel(dev)
    record("forward.xent", o)
    assert o["lp_abs"] < XENT_ABS and o["lse_excess"] < XENT_ABS, o
    assert o["bitwise"] and o["ignored_zero"], o


def _llama8b_2layer():
    return opa.OpusConfig(enc_layers=1, enc_dim=64, enc_heads=4, enc_ffn=256, proj_dim=64,
                          dec_layers=2, dec_dim=4096, dec_heads=32, dec_kv_heads=8, dec_head_dim=128, dec_ffn=14336,
                          dec_vocab=128256, dec_rope_theta=500000.0, max_batch=8, max_enc_tokens=66, max_prompt=48,
                          max_new_tokens=4).validate()


def _check_oracle(o, lp=LP_ABS_ORACLE, loss=LOSS_REL_ORACLE, logits=REL_L2, paths=PATHS_ABS, ulp=ULP_REL):
    assert o["lp_abs"] < lp and o["lossonly_lp_abs"] < lp, o
    assert o["loss_rel"] < loss and o["lossonly_loss_rel"] < loss, o
    assert o["logits_rel_l2"] < logits, o
    assert o["paths_abs"] < max(paths, 2 * ulp * o["logit_absmax"]), o
    assert o["lossonly_bitwise"] and o["zero_elsewhere"] and o["n_tokens_ok"] and o["logits_none"], o


def test_llama3_8b_widths_two_layers_vs_oracle(dev):
    """Full Llama-3-8B widths (V = 128 256: lm_head over rows at gemm_pp size), 2 layers, batch 8 of right-padded rows."""
    o = fc.vs_oracle(dev, _llama8b_2layer(), B=8, T=40)
    record("forward.llama8b_2layer", o)
    _check_oracle(o)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,cfg", [
    ("qwen2", opa.micro_qwen()),
    ("opt", opa.micro_opt()),
    ("opt_relu_v50272", opa.micro_opt_relu(dec_vocab=50272)),
    ("llama_v151936", opa.micro(dec_vocab=151936)),
    ("opt_v50000", opa.micro_opt(dec_vocab=50000)),
])
def test_families_and_vocab_widths_vs_oracle(dev, name, cfg):
    """Qwen2 (q/k/v biases) and OPT (LayerNorm + lm_head_opt) micro decoders, and vocabularies that are not multiples of 256
    through the lm_head over 6 x 40 rows (gemm_pp / tile routing of the M-row lm_head)."""
    o = fc.vs_oracle(dev, cfg, B=6, T=40, seed=1)
    record("forward.family." + name, o)
    _check_oracle(o)


def test_batches_above_max_batch_and_rows_alone(dev):
    """2 max_batch + 3 rows (three groups) against the same rows in one larger-capacity context, rows scored alone against their
    row of the batch, left-padded rows (with position_ids) against right-padded ones - at Llama-3-8B widths, 2 layers."""
    cfg = _llama8b_2layer()
    big = opa.OpusConfig(**{**cfg.__dict__, "max_batch": 32}).validate()
    m8, m32 = fc.make_model(cfg, dev), fc.make_model(big, dev)
    B, T = 2 * cfg.max_batch + 3, 40
    ids, mask, labels = fc._text_batch(cfg, B, T, seed=3)
    obs = {}
    for rl in (False, True):
        a = m8(ids, attention_mask=mask, labels=labels, return_logits=rl)
        b = m32(ids, attention_mask=mask, labels=labels, return_logits=rl)
        assert a.n_tokens == b.n_tokens
        obs[f"loss_rel_{rl}"] = abs(float(a.loss) - float(b.loss)) / abs(float(b.loss))
        obs[f"token_abs_{rl}"] = float((a.token_logprobs - b.token_logprobs).abs().max())
    whole = m32(ids, attention_mask=mask, labels=labels, return_logits=False)
    obs["alone_abs"] = 0.0
    for r in (0, 5, B - 1):
        one = m8(ids[r:r + 1], attention_mask=mask[r:r + 1], labels=labels[r:r + 1], return_logits=False)
        obs["alone_abs"] = max(obs["alone_abs"], float((one.token_logprobs[0] - whole.token_logprobs[r]).abs().max()))
    # left-padded rows with position_ids = cumsum(mask) - 1: the same scores as the right-padded rows
    lids, lmask, llab = torch.full_like(ids, 2), torch.zeros_like(mask), torch.full_like(labels, -100)
    for r in range(B):
        n = int(mask[r].sum())
        lids[r, T - n:], lmask[r, T - n:], llab[r, T - n:] = ids[r, :n], True, labels[r, :n]
    pos = (lmask.long().cumsum(-1) - 1).clamp(min=0)
    left = m32(lids, attention_mask=lmask, labels=llab, position_ids=pos, return_logits=False)
    obs["left_loss_rel"] = abs(float(left.loss) - float(whole.loss)) / abs(float(whole.loss))
    record("forward.batches", obs)
    # one loss over all groups; per token, the groups run the layers at other row counts (other GEMM kernels): the oracle bound
    assert obs["loss_rel_False"] < 2e-3 and obs["loss_rel_True"] < 2e-3, obs
    assert obs["token_abs_False"] < LP_ABS_ORACLE and obs["token_abs_True"] < LP_ABS_ORACLE, obs
    # a row alone runs every layer at 40 rows (mid / stream kernels) instead of 19 x 40 (gemm_pp): fp16 hand-offs of other kernels,
    # observed 6.2e-3 on MI355X (the same row in the two batch shapes above: 9.1e-3); bound ~2.5 x
    assert obs["alone_abs"] < ROW_ALONE_ABS, obs
    assert obs["left_loss_rel"] < 2e-3, obs
    del m8, m32
    torch.cuda.empty_cache()


def test_context_state_and_errors(dev):
    cfg = opa.micro()
    model = fc.make_model(cfg, dev)
    ids, mask, labels = fc._text_batch(cfg, 3, 20, seed=5)
    gen = dict(attention_mask=torch.ones_like(ids, dtype=torch.bool), pad_token_id=2, do_sample=False, max_new_tokens=8)
    before = model.generate(ids, **gen).cpu()
    out = model(ids, attention_mask=mask, labels=labels)
    assert torch.isfinite(out.loss)
    with pytest.raises(_cabi.OpusError) as e:
        model.decode_logits(torch.zeros(3, dtype=torch.int32))
    assert e.value.code == -6                                   # OPUS_ESTATE
    after = model.generate(ids, **gen).cpu()
    assert torch.equal(before, after)
    # HF-shaped result
    assert out["loss"] is out.loss and out[0] is out.loss and out[1] is out.logits and out.past_key_values is None
    tup = model(ids, attention_mask=mask, labels=labels, return_dict=False)
    assert len(tup) == 2 and torch.equal(tup[0], out.loss)
    assert len(model(ids, attention_mask=mask, return_dict=False)) == 1          # (loss None is dropped)
    nan = model(ids, attention_mask=mask, labels=torch.full_like(labels, -100))
    assert nan.n_tokens == 0 and torch.isnan(nan.loss)
    # errors
    long = torch.full((1, cfg.max_prompt + 1), 5, dtype=torch.long)
    with pytest.raises(_cabi.OpusError) as e:
        model(long, labels=long)
    assert e.value.code == -2                                   # OPUS_ESHAPE
    hole = mask.clone()
    hole[0, 3] = False
    with pytest.raises(ValueError, match="hole"):
        model(ids, attention_mask=hole, labels=labels)
    left = torch.zeros_like(mask)
    left[:, 4:] = True
    with pytest.raises(ValueError, match="position_ids"):
        model(ids, attention_mask=left)
    with pytest.raises(NotImplementedError):
        model(ids, attention_mask=mask, past_key_values=((None, None),))
    with pytest.raises(NotImplementedError):
        model(ids, attention_mask=mask, use_cache=True)
    with pytest.raises(NotImplementedError):
        model(ids, attention_mask=mask, output_hidden_states=True)


def test_loss_only_memory_is_bounded(dev):
    """Loss-only scoring at Llama-3-8B widths: the logits slab is chunked, so the extra device memory of a call does not grow with
    the number of scored rows."""
    cfg = _llama8b_2layer()
    model = fc.make_model(cfg, dev)
    ids, mask, labels = fc._text_batch(cfg, 8, 48, seed=7)
    model(ids, attention_mask=mask, labels=labels, return_logits=False)        # (warm: allocator pools)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    model(ids, attention_mask=mask, labels=labels, return_logits=False)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - base
    assert extra < 512 * 2 ** 20, extra
    del model
    torch.cuda.empty_cache()


def test_bf16_build_forward():
    env = dict(os.environ, OPUS_DTYPE="bf16")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bf16_forward_check.py")], capture_output=True, text=True,
                       env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("BF16_FORWARD ")][-1]
    o = json.loads(line[len("BF16_FORWARD "):])
    record("forward.bf16", o)
    assert o["operand_dtype"] == 1, o
    for tag, g in o["golden"].items():                       # bounds: 8 x the fp16 ones
        assert g["shape_ok"] and g["logits_rel_l2"] < 8 * REL_L2, (tag, g)
        if tag != "d":
            assert g["loss_rel"] < 8 * LOSS_REL_GOLD and g["lp_abs"] < 8 * LP_ABS_GOLD and g["n_tokens_ok"], (tag, g)
    x = o["xent"]
    assert x["lp_abs"] < XENT_ABS and x["lse_excess"] < XENT_ABS and x["bitwise"] and x["ignored_zero"], x
    _check_oracle(o["llama8b"], lp=8 * LP_ABS_ORACLE, loss=8 * LOSS_REL_ORACLE, logits=8 * REL_L2, paths=8 * PATHS_ABS,
                  ulp=2.0 ** -7)
