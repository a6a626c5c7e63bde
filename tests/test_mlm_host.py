"""ESM-2 masked-LM head, host side (no GPU): the restated head against transformers' EsmForMaskedLM and the fixture
tests/golden/mlm_micro.npz, the checkpoint mapping, the synthetic head, mutation strings, the plan of masked copies and the C ABI
declarations."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, alphabet, mlm, synth
from opus_pllm_amd.builder import canonical_from_esm2, mlm_head_from_esm2
import mlm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_ABS = 2e-5                     # the project's bound for fp32 fixtures
NEW_SYMBOLS = ("opus_esm2_lm_head", "opus_debug_esm2_lm_head")


@pytest.fixture(scope="module")
def micro():
    cfg = opa.micro()
    return cfg, synth.canonical_weights(cfg, 0), synth.mlm_head(cfg, 0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "mlm_micro.npz"))


# ------------------------------------------------------------------------------------------------ restatement
def test_restated_head_equals_transformers(micro):
    pytest.importorskip("transformers")
    cfg, W, head = micro
    hf = mlm_ref.build_hf_mlm(cfg, W, head)
    toks = mlm_ref.fixture_tokens()
    assert toks.shape == (3, 4, 66) and [int((t != 1).sum()) - 2 for t in toks[0]] == [1, 2, 17, 64]
    assert [int((v == 32).sum()) for v in toks] == [0, 4, int((toks[2] == 32).sum())] and (toks[2] == 32).sum(1).max() >= 3
    for v in toks:
        t = torch.from_numpy(v).long()
        real = t != 1
        ref = mlm_ref.hf_logits(hf, t)
        got = mlm_ref.model_logits(t, W, cfg, head)
        assert float((got[real] - ref[real]).abs().max()) <= FP32_ABS
    # an untied output projection is a separate table in both
    untied = synth.mlm_head(cfg, 0, tied=False)
    hf2 = mlm_ref.build_hf_mlm(cfg, W, untied)
    t = torch.from_numpy(toks[1]).long()
    a, b = mlm_ref.model_logits(t, W, cfg, untied), mlm_ref.hf_logits(hf2, t)
    assert float((a - b)[t != 1].abs().max()) <= FP32_ABS
    assert float((a - mlm_ref.model_logits(t, W, cfg, head))[t != 1].abs().max()) > 0.1


def test_fixture_keeps_its_promises(micro, gold):
    cfg, W, head = micro
    assert int(gold["head_seed"]) == 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mlm_micro.npz")) < 153 * 1024
    toks = gold["tokens"]
    assert np.array_equal(toks, mlm_ref.fixture_tokens())
    assert gold["logits"].shape == (3, 4, 66, 33) and gold["logits"].dtype == np.float32
    real = toks != 1
    std = float(gold["logits"][real].std(axis=-1).mean())
    assert abs(std - float(gold["logit_std"])) < 1e-6 and std > 0.5            # a near-constant head tests nothing
    for v in range(3):
        t = torch.from_numpy(toks[v]).long()
        got = mlm_ref.model_logits(t, W, cfg, head)
        assert float((got - torch.from_numpy(gold["logits"][v]))[t != 1].abs().max()) <= FP32_ABS
    fn = mlm_ref.oracle_logits_fn(W, cfg, head)
    for i, s in enumerate(mlm_ref.scan_sequences()):
        ids = mlm_ref.ids_of(s)
        assert np.array_equal(gold[f"scan_tokens_{i}"], ids) and len(ids) == mlm_ref.SCAN_LENGTHS[i]
        lp = mlm_ref.masked_marginals(ids, fn)
        ref = torch.from_numpy(gold[f"scan_log_probs_{i}"]).double()
        assert float((lp - ref).abs().max()) <= FP32_ABS
        assert float((torch.logsumexp(ref, -1)).abs().max()) < 1e-5            # rows are log-probabilities
        # masking a residue changes its row: the scan is not the one-pass table
        assert float((lp - mlm_ref.wt_marginals(ids, fn)).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------------ checkpoint mapping
def _esm_sd(cfg, W, head, prefix, lm_weight="tied"):
    sd = {"embed_tokens.weight": torch.from_numpy(W["enc.embed_tokens"]),
          "emb_layer_norm_after.weight": torch.from_numpy(W["enc.ln_f.weight"]),
          "emb_layer_norm_after.bias": torch.from_numpy(W["enc.ln_f.bias"])}
    for l in range(cfg.enc_layers):
        s, d = f"layers.{l}.", f"enc.layers.{l}."
        for a, b in (("ln1", "self_attn_layer_norm"), ("q", "self_attn.q_proj"), ("k", "self_attn.k_proj"),
                     ("v", "self_attn.v_proj"), ("o", "self_attn.out_proj"), ("ln2", "final_layer_norm"),
                     ("fc1", "fc1"), ("fc2", "fc2")):
            sd[s + b + ".weight"] = torch.from_numpy(W[d + a + ".weight"])
            sd[s + b + ".bias"] = torch.from_numpy(W[d + a + ".bias"])
    if head is not None:
        for a, b in (("dense.weight", "dense.weight"), ("dense.bias", "dense.bias"), ("layer_norm.weight", "ln.weight"),
                     ("layer_norm.bias", "ln.bias"), ("bias", "bias")):
            sd["lm_head." + a] = torch.from_numpy(head["enc.lm." + b])
        if lm_weight == "tied":
            sd["lm_head.weight"] = sd["embed_tokens.weight"].clone()
        elif lm_weight == "untied":
            sd["lm_head.weight"] = sd["embed_tokens.weight"] + 0.5
    return {prefix + k: v for k, v in sd.items()}


@pytest.mark.parametrize("prefix", ["encoder.sentence_encoder.", "encoder.", "sentence_encoder.", ""])
def test_mlm_head_from_esm2(micro, prefix):
    cfg, W, head = micro
    sd = _esm_sd(cfg, W, head, prefix)
    got = mlm_head_from_esm2(sd)
    assert set(got) == set(synth.MLM_HEAD_NAMES)                               # tied: no table of its own
    for k in got:
        assert got[k].dtype == torch.float32 and np.array_equal(got[k].numpy(), head[k])
    assert tuple(got["enc.lm.dense.weight"].shape) == (cfg.enc_dim, cfg.enc_dim) and tuple(got["enc.lm.bias"].shape) == (33,)
    assert mlm_head_from_esm2(_esm_sd(cfg, W, None, prefix)) is None
    un = mlm_head_from_esm2(_esm_sd(cfg, W, head, prefix, "untied"))
    assert set(un) == set(synth.MLM_HEAD_NAMES) | {"enc.lm.weight"}
    assert np.allclose(un["enc.lm.weight"].numpy(), W["enc.embed_tokens"] + 0.5)
    assert set(mlm_head_from_esm2(_esm_sd(cfg, W, head, prefix, "absent"))) == set(synth.MLM_HEAD_NAMES)
    assert not any(".lm." in k for k in canonical_from_esm2(sd, cfg))          # the encoder loader is unchanged


# ------------------------------------------------------------------------------------------------ synthetic head
def test_synthetic_head():
    cfg = opa.micro()
    a, b, c = synth.mlm_head(cfg, 0), synth.mlm_head(cfg, 0), synth.mlm_head(cfg, 1)
    assert set(a) == set(synth.MLM_HEAD_NAMES)
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert all(not np.array_equal(a[k], c[k]) for k in a)
    for name, shape, std, mean in synth.mlm_head_spec(cfg):                    # each tensor from its own stream
        assert a[name].shape == shape
        assert np.array_equal(a[name].ravel()[:5], synth.hash_normal(synth.tensor_seed(name, 0), 0, 5, std, mean))
    assert "enc.lm.weight" in synth.mlm_head(cfg, 0, tied=False)
    names = [n for n, _, _, _ in synth.canonical_spec(cfg)]
    assert not any(".lm." in n for n in names)
    assert synth.param_count(cfg) == sum(int(np.prod(s)) for _, s, _, _ in synth.canonical_spec(cfg))
    from opus_pllm_amd.weights import DeviceWeights
    assert inspect.signature(DeviceWeights.synthetic).parameters["mlm_head"].default is False
    assert inspect.signature(DeviceWeights.synthetic).parameters["contact_head"].default is False


def test_standard_residue_columns():
    assert len(alphabet.STANDARD_RESIDUE_IDS) == 20 == len(set(alphabet.STANDARD_RESIDUE_IDS))
    assert [alphabet.ALL_TOKS[i] for i in alphabet.STANDARD_RESIDUE_IDS] == list("ACDEFGHIKLMNPQRSTVWY")
    assert all(4 <= i <= 23 for i in alphabet.STANDARD_RESIDUE_IDS)


# ------------------------------------------------------------------------------------------------ mutation strings
def test_parse_mutation():
    ids = alphabet.encode_array("MKTAYIAK")
    A, G, M, K = (alphabet.TOK_TO_IDX[c] for c in "AGMK")
    assert mlm.parse_mutation("A4G", ids) == [(3, A, G)]
    assert mlm.parse_mutation("A3G", ids, offset_idx=0) == [(3, A, G)]
    assert mlm.parse_mutation("M24G", ids, offset_idx=24) == [(0, M, G)]
    assert mlm.parse_mutation("M1K:K8M", ids) == [(0, M, K), (7, K, M)]
    with pytest.raises(ValueError, match=re.escape("'G4A'") + ".*does not match"):
        mlm.parse_mutation("G4A", ids)
    with pytest.raises(ValueError, match=re.escape("'A9G'") + ".*out of range"):
        mlm.parse_mutation("A9G", ids)
    with pytest.raises(ValueError, match=re.escape("'M0G'") + ".*out of range"):
        mlm.parse_mutation("M0G", ids)
    with pytest.raises(ValueError, match=re.escape("'A4J'") + ".*not in the alphabet"):
        mlm.parse_mutation("A4J", ids)
    with pytest.raises(ValueError, match=re.escape("'M1K:A9G'") + ".*out of range"):
        mlm.parse_mutation("M1K:A9G", ids)
    with pytest.raises(ValueError, match="A4"):
        mlm.parse_mutation("A4", ids)


def test_additive_rule_and_positions_from_mutations():
    ids = [alphabet.encode_array("MKTAYIAK"), alphabet.encode_array("ACD")]
    parsed = [[mlm.parse_mutation(m, ids[0]) for m in ("A4G", "M1K:K8M", "K8M")], []]
    assert mlm.scan_positions([8, 3], None, parsed) == [[0, 3, 7], []]
    assert mlm.scan_positions([8, 3], None, None) == [list(range(8)), [0, 1, 2]]
    assert mlm.scan_positions([8, 3], [[5, 1, 5], [2]], parsed) == [[1, 5], [2]]       # explicit positions win
    with pytest.raises(ValueError, match="positions"):
        mlm.scan_positions([8, 3], [[8], []], None)
    # a multiple mutation is the sum of its parts
    scores = torch.arange(8 * 33, dtype=torch.float32).reshape(8, 33)
    multi = sum(scores[i, mt] for i, _, mt in parsed[0][1])
    assert float(multi) == float(scores[0, alphabet.TOK_TO_IDX["K"]] + scores[7, alphabet.TOK_TO_IDX["M"]])


# ------------------------------------------------------------------------------------------------ copy planning
def test_plan_masked_copies():
    mb, mt = 8, 66

    def plan(lengths, scan=None):
        scan = scan or [list(range(n)) for n in lengths]
        p = mlm.plan_masked_copies(scan, lengths, mb, mt)
        copies = sum(len(s) for s in scan)
        assert len(p) == math.ceil(copies / mb) and sum(len(c) for c in p) == copies       # encoder_calls, rows_evaluated
        assert all(1 <= len(c) <= mb for c in p)
        assert [c for call in p for c in call] == [(i, j) for i, s in enumerate(scan) for j in s]
        return p
    assert len(plan([mb])) == 1                                 # max_batch copies: one call
    assert len(plan([mb + 1])) == 2                             # one more: two
    p = plan([3, 4])                                            # two proteins share a call
    assert len(p) == 1 and {i for i, _ in p[0]} == {0, 1}
    p = plan([mt - 2])                                          # the longest protein the encoder takes
    assert len(p) == math.ceil((mt - 2) / mb)
    with pytest.raises(ValueError, match="max_enc_tokens"):
        mlm.plan_masked_copies([[0]], [mt - 1], mb, mt)
    assert plan([5, 6], [[], [1, 4]]) == [[(1, 1), (1, 4)]]
    assert mlm.plan_masked_copies([[], []], [5, 6], mb, mt) == []
    c = mlm.masked_copy(np.array([5, 6, 7], dtype=np.int32), 1)
    assert c.tolist() == [5, 32, 7]


# ------------------------------------------------------------------------------------------------ C ABI
def test_abi_entries():
    hdr = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    assert "#define OPUS_ABI_VERSION 10" in hdr
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_cabi.SIGNATURES[name][1]) == 6
    assert _cabi.ABI_VERSION == 10
    lib = _cabi.lib()
    assert lib.opus_abi_version() == 10
    libdir = os.path.dirname(_cabi.LIB_PATH)
    for so in ("libopus_pllm.so", "libopus_pllm_bf16.so"):
        l = C.CDLL(os.path.join(libdir, so))
        for name in NEW_SYMBOLS:
            assert hasattr(l, name), (so, name)
    out = (C.c_float * 33)()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name)(None, None, 1, 0, out, None) == -1            # OPUS_EBADARG: null context
        assert b"ctx is null" in lib.opus_last_error()
    buf = C.create_string_buffer(512)
    assert lib.opus_timing_names(buf, 512) == 0
    classes = buf.value.decode().split(";")[0].split(",")
    assert classes[-2:] == ["logitproc", "xent"] and classes[-3] == "mlm"
    assert "contact" in classes and "constraint" in classes
