"""ESM-2 contact maps, host side (no GPU): the rank-1 reformulation the kernels use against transformers'
EsmContactPredictionHead, the fair-esm contact-head loader, the synthetic head and the C ABI declarations."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth
from opus_pllm_amd.builder import canonical_from_esm2, contact_head_from_esm2
import contact_checks as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stack(lens, L, H, seed):
    """Padded ragged batch: tokens [B, T] (<cls> residues <eos> <pad>...) and softmax attention [B, L, H, T, T] over each
    protein's own keys (padding keys masked, as the encoder does)."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens) + 2
    tok = torch.ones(B, T, dtype=torch.long)
    for b, n in enumerate(lens):
        tok[b, 0] = 0
        tok[b, 1:n + 1] = torch.randint(4, 24, (n,), generator=g)
        tok[b, n + 1] = 2
    s = torch.randn(B, L, H, T, T, generator=g, dtype=torch.float64) * 2.0
    key_pad = (tok == 1)[:, None, None, None, :]
    return tok, torch.softmax(s.masked_fill(key_pad, float("-inf")), -1)


def test_reformulation_equals_hf_head():
    lens, L, H = [0, 1, 2, 9, 23, 5], 3, 4
    tok, attn = _stack(lens, L, H, seed=1)
    g = torch.Generator().manual_seed(2)
    w, bias = torch.randn(L * H, generator=g, dtype=torch.float64) * 3.0, torch.tensor([0.3], dtype=torch.float64)
    ref = cc.hf_contacts(tok, attn, w.numpy(), bias.numpy())
    assert ref.shape == (len(lens), max(lens), max(lens))
    for b, n in enumerate(lens):
        rf = cc.Reform(n, w.numpy(), bias.numpy())
        for l in range(L):
            rf.add_layer(attn[b, l, :, :n + 2, :n + 2])
        got = rf.contacts()
        assert got.shape == (n, n)
        if n:
            assert torch.allclose(got, ref[b, :n, :n], atol=1e-12, rtol=0), (b, (got - ref[b, :n, :n]).abs().max())
            assert float(rf.logits().std() if n > 1 else 1.0) > 0.0


def _esm_sd(cfg, with_head):
    w = synth.canonical_weights(cfg, 0)
    sd = {"embed_tokens.weight": torch.from_numpy(w["enc.embed_tokens"]),
          "emb_layer_norm_after.weight": torch.from_numpy(w["enc.ln_f.weight"]),
          "emb_layer_norm_after.bias": torch.from_numpy(w["enc.ln_f.bias"])}
    for l in range(cfg.enc_layers):
        s, d = f"layers.{l}.", f"enc.layers.{l}."
        for a, b in (("ln1", "self_attn_layer_norm"), ("q", "self_attn.q_proj"), ("k", "self_attn.k_proj"),
                     ("v", "self_attn.v_proj"), ("o", "self_attn.out_proj"), ("ln2", "final_layer_norm"),
                     ("fc1", "fc1"), ("fc2", "fc2")):
            sd[s + b + ".weight"] = torch.from_numpy(w[d + a + ".weight"])
            sd[s + b + ".bias"] = torch.from_numpy(w[d + a + ".bias"])
    if with_head:
        C_ = cfg.enc_layers * cfg.enc_heads
        sd["contact_head.regression.weight"] = torch.arange(C_, dtype=torch.float32).reshape(1, C_)
        sd["contact_head.regression.bias"] = torch.tensor([0.25])
    return {"encoder.sentence_encoder." + k: v for k, v in sd.items()}


def test_contact_head_from_esm2():
    cfg = opa.micro()
    sd = _esm_sd(cfg, True)
    head = contact_head_from_esm2(sd)
    assert set(head) == {"enc.contact.weight", "enc.contact.bias"}
    assert head["enc.contact.weight"].dtype == torch.float32 and tuple(head["enc.contact.weight"].shape) == (8,)
    assert torch.equal(head["enc.contact.weight"], torch.arange(8, dtype=torch.float32))
    assert tuple(head["enc.contact.bias"].shape) == (1,) and float(head["enc.contact.bias"]) == 0.25
    assert contact_head_from_esm2(_esm_sd(cfg, False)) is None
    assert not any("contact" in k for k in canonical_from_esm2(sd, cfg))      # the encoder loader is unchanged


def test_synth_contact_head():
    cfg = opa.micro()
    a, b = synth.contact_head(cfg, 0), synth.contact_head(cfg, 0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["enc.contact.weight"].shape == (cfg.enc_layers * cfg.enc_heads,) and a["enc.contact.bias"].shape == (1,)
    assert a["enc.contact.weight"].dtype == np.float32
    assert not np.array_equal(synth.contact_head(cfg, 1)["enc.contact.weight"], a["enc.contact.weight"])
    assert abs(float(a["enc.contact.weight"].std()) - synth.contact_head_std(cfg)) < 0.6 * synth.contact_head_std(cfg)
    names = [n for n, _, _, _ in synth.canonical_spec(cfg)]
    assert not any("contact" in n for n in names)
    assert synth.param_count(cfg) == sum(int(np.prod(s)) for _, s, _, _ in synth.canonical_spec(cfg))


def test_golden_contacts_fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "contacts_micro.npz"))
    cfg = opa.micro()
    head = synth.contact_head(cfg, 0)
    assert np.array_equal(g["weight"], head["enc.contact.weight"]) and np.array_equal(g["bias"], head["enc.contact.bias"])
    assert float(g["logit_std"]) > 0.5
    c = g["contacts"]
    for i, n in enumerate(g["lens"] - 2):
        blk = c[i, :n, :n]
        assert np.allclose(blk, blk.T, atol=1e-6) and ((blk > 0) & (blk < 1)).all()


def test_abi_entries():
    for name in ("opus_esm2_contacts_packed", "opus_esm2_contacts_scratch_bytes", "opus_debug_contacts"):
        assert name in _cabi.SIGNATURES
    assert _cabi.ABI_VERSION == 10
    lib = _cabi.lib()
    cc_ = _cabi.CConfig.from_config(opa.micro())
    cu = (C.c_int32 * 4)(0, 19, 21, 87)                    # 17, 0 and 64 residues
    n2, ni, C_ = 17 * 17 + 64 * 64, 17 + 64, 8
    pq = 17 + 64
    al = lambda v: (v + 255) // 256 * 256                  # noqa: E731
    exp = al(4 * n2) + al(4 * ni * C_) + al(4 * 4 * pq) + al(4 * 3 * C_)
    assert lib.opus_esm2_contacts_scratch_bytes(C.byref(cc_), cu, 3) == exp
    bad = (C.c_int32 * 2)(0, 1)                            # fewer than 2 tokens
    assert lib.opus_esm2_contacts_scratch_bytes(C.byref(cc_), bad, 1) == -1
    buf = C.create_string_buffer(512)
    assert lib.opus_timing_names(buf, 512) == 0
    assert "contact" in buf.value.decode().split(";")[0].split(",")


def _head_file(path, C_, wrap=True):
    sd = {"contact_head.regression.weight": torch.arange(C_, dtype=torch.float32).reshape(1, C_) / 10,
          "contact_head.regression.bias": torch.tensor([-0.5])}
    torch.save({"model": sd} if wrap else sd, path)


def test_esm2_contact_head_two_file_layout(tmp_path, monkeypatch):
    """fair-esm's layout: the ESM-2 checkpoint without the regression + <stem>-contact-regression.pt beside it."""
    from opus_pllm_amd.builder import esm2_contact_ckpt_path, load_esm2_contact_head
    monkeypatch.delenv("OPUS_ESM2_CONTACT_CKPT", raising=False)
    cfg = opa.micro()
    main = tmp_path / "esm2_t33_650M_UR50D.pt"
    sd = _esm_sd(cfg, False)
    torch.save({"model": sd}, main)
    assert esm2_contact_ckpt_path(str(main)) is None and load_esm2_contact_head(str(main), sd) is None
    _head_file(tmp_path / "esm2_t33_650M_UR50D-contact-regression.pt", 8)
    assert esm2_contact_ckpt_path(str(main)) == str(tmp_path / "esm2_t33_650M_UR50D-contact-regression.pt")
    head = load_esm2_contact_head(str(main), torch.load(main, weights_only=False)["model"])
    assert torch.equal(head["enc.contact.weight"], torch.arange(8, dtype=torch.float32) / 10)
    assert float(head["enc.contact.bias"]) == -0.5
    # the head inside the checkpoint itself wins over the sibling file
    assert float(load_esm2_contact_head(str(main), _esm_sd(cfg, True))["enc.contact.bias"]) == 0.25
    # an explicit file wins over both; a missing one, or one without the tensors, raises
    other = tmp_path / "elsewhere.pt"
    _head_file(other, 8, wrap=False)
    monkeypatch.setenv("OPUS_ESM2_CONTACT_CKPT", str(other))
    assert float(load_esm2_contact_head(str(main), _esm_sd(cfg, True))["enc.contact.bias"]) == -0.5
    monkeypatch.setenv("OPUS_ESM2_CONTACT_CKPT", str(tmp_path / "missing.pt"))
    with pytest.raises(FileNotFoundError):
        load_esm2_contact_head(str(main), sd)
    torch.save({"model": {"x": torch.zeros(1)}}, tmp_path / "empty.pt")
    monkeypatch.setenv("OPUS_ESM2_CONTACT_CKPT", str(tmp_path / "empty.pt"))
    with pytest.raises(ValueError, match="contact_head.regression"):
        load_esm2_contact_head(str(main), sd)


def test_synthetic_head_is_opt_in():
    import inspect
    from opus_pllm_amd.weights import DeviceWeights
    assert inspect.signature(DeviceWeights.synthetic).parameters["contact_head"].default is False
