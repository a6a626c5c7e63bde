"""Test infrastructure for the ESM-2 masked-LM head (get_residue_logits / score_mutations): the head restated on top of the
fp32 encoder oracle (oracle.esm2.esm2_hidden, import only), transformers' EsmForMaskedLM carrying the same tensors, and the two
scoring strategies of fair-esm's examples/variant-prediction/predict.py as plain loops over any `logits_fn`.

    logits = LayerNorm(gelu_erf(h Wd^T + bd)) We^T + b        (RobertaLMHead / EsmLMHead; We = the token embedding when tied)
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from opus_pllm_amd import synth
from opus_pllm_amd.alphabet import MASK_IDX, PAD_IDX, batch_convert, encode_array

LN_EPS = 1e-5


def _t(v, dtype):
    return (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(dtype)


def head_logits(hidden: torch.Tensor, head: Dict, emb, eps: float = LN_EPS, dtype=torch.float64) -> torch.Tensor:
    """The head on states [..., De] in `dtype` (fp64: the reference of the kernel tests; fp32: the restatement of the libraries)."""
    h = hidden.to(dtype)
    y = F.linear(h, _t(head["enc.lm.dense.weight"], dtype), _t(head["enc.lm.dense.bias"], dtype))
    y = y * 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0)))
    y = F.layer_norm(y, (y.shape[-1],), _t(head["enc.lm.ln.weight"], dtype), _t(head["enc.lm.ln.bias"], dtype), eps)
    we = _t(head["enc.lm.weight"] if "enc.lm.weight" in head else emb, dtype)
    return F.linear(y, we, _t(head["enc.lm.bias"], dtype))


def model_logits(tokens: torch.Tensor, W, cfg, head, dtype=torch.float32) -> torch.Tensor:
    """tokens int64 [B, T] (padded with <pad>) -> logits [B, T, 33]: the fp32 encoder oracle, then the head in `dtype`."""
    from oracle.esm2 import esm2_hidden
    with torch.no_grad():
        hid = esm2_hidden(tokens, {k: _t(W[k], torch.float32) for k in W}, cfg)
        return head_logits(hid, head, W["enc.embed_tokens"], cfg.enc_ln_eps, dtype)


def oracle_logits_fn(W, cfg, head, dtype=torch.float32) -> Callable:
    """logits_fn for the loops below: residue ids [n] -> [n, 33] of that protein alone."""
    Wt = {k: _t(W[k], torch.float32) for k in W}

    def fn(ids: np.ndarray) -> torch.Tensor:
        from oracle.esm2 import esm2_hidden
        toks = torch.tensor([[0] + [int(v) for v in ids] + [2]], dtype=torch.long)
        with torch.no_grad():
            hid = esm2_hidden(toks, Wt, cfg)
            return head_logits(hid[0, 1:-1], head, Wt["enc.embed_tokens"], cfg.enc_ln_eps, dtype)
    return fn


# ------------------------------------------------------------------------------------------------ transformers
def build_hf_mlm(cfg, W, head):
    """transformers' EsmForMaskedLM (rotary, token_dropout=True, mask id 32, pad id 1) carrying the canonical tensors W + head."""
    from transformers import EsmConfig, EsmForMaskedLM
    ec = EsmConfig(vocab_size=cfg.enc_vocab, hidden_size=cfg.enc_dim, num_hidden_layers=cfg.enc_layers,
                   num_attention_heads=cfg.enc_heads, intermediate_size=cfg.enc_ffn, position_embedding_type="rotary",
                   token_dropout=True, emb_layer_norm_before=False, pad_token_id=1, mask_token_id=32, layer_norm_eps=cfg.enc_ln_eps,
                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, tie_word_embeddings="enc.lm.weight" not in head)
    ec._attn_implementation = "eager"
    m = EsmForMaskedLM(ec).eval()
    f = lambda v: _t(v, torch.float32)          # noqa: E731
    sd = {"esm.embeddings.word_embeddings.weight": f(W["enc.embed_tokens"]),
          "esm.encoder.emb_layer_norm_after.weight": f(W["enc.ln_f.weight"]), "esm.encoder.emb_layer_norm_after.bias": f(W["enc.ln_f.bias"]),
          "lm_head.dense.weight": f(head["enc.lm.dense.weight"]), "lm_head.dense.bias": f(head["enc.lm.dense.bias"]),
          "lm_head.layer_norm.weight": f(head["enc.lm.ln.weight"]), "lm_head.layer_norm.bias": f(head["enc.lm.ln.bias"]),
          "lm_head.bias": f(head["enc.lm.bias"]),
          "lm_head.decoder.weight": f(head["enc.lm.weight"] if "enc.lm.weight" in head else W["enc.embed_tokens"])}
    for l in range(cfg.enc_layers):
        s, d = f"enc.layers.{l}.", f"esm.encoder.layer.{l}."
        for a, b in (("ln1", "attention.LayerNorm"), ("q", "attention.self.query"), ("k", "attention.self.key"),
                     ("v", "attention.self.value"), ("o", "attention.output.dense"), ("ln2", "LayerNorm"),
                     ("fc1", "intermediate.dense"), ("fc2", "output.dense")):
            sd[d + b + ".weight"] = f(W[s + a + ".weight"])
            sd[d + b + ".bias"] = f(W[s + a + ".bias"])
    missing, unexpected = m.load_state_dict(sd, strict=False)
    bad = [k for k in missing if not any(t in k for t in ("inv_freq", "position_embeddings", "position_ids", "contact_head", "lm_head.decoder.bias"))]
    assert not bad and not unexpected, (bad, unexpected)
    with torch.no_grad():
        if getattr(m.lm_head.decoder, "bias", None) is not None and m.lm_head.decoder.bias is not m.lm_head.bias:
            m.lm_head.decoder.bias.zero_()
    return m


def hf_logits(hf, tokens: torch.Tensor) -> torch.Tensor:
    with torch.no_grad():
        return hf(input_ids=tokens, attention_mask=(tokens != PAD_IDX).long()).logits.float()


def hf_logits_fn(hf) -> Callable:
    def fn(ids: np.ndarray) -> torch.Tensor:
        toks = torch.tensor([[0] + [int(v) for v in ids] + [2]], dtype=torch.long)
        return hf_logits(hf, toks)[0, 1:-1]
    return fn


# ------------------------------------------------------------------------------------------------ the two strategies
def wt_marginals(ids: np.ndarray, logits_fn: Callable) -> torch.Tensor:
    """log p(token at j | the unmasked protein), [n, 33]: one pass."""
    return torch.log_softmax(logits_fn(np.asarray(ids)).double(), -1)


def masked_marginals(ids: np.ndarray, logits_fn: Callable, positions: Sequence[int] = None) -> torch.Tensor:
    """Row j = log-softmax of row j of the pass over the copy whose residue j is <mask>; rows outside `positions` NaN."""
    ids = np.asarray(ids)
    n = len(ids)
    out = torch.full((n, 33), float("nan"), dtype=torch.float64)
    for j in (range(n) if positions is None else positions):
        c = ids.copy()
        c[j] = MASK_IDX
        out[j] = torch.log_softmax(logits_fn(c)[j].double(), -1)
    return out


def summarize(log_probs: torch.Tensor, ids: np.ndarray):
    """(wt_log_prob [n], pseudo log-likelihood, pseudo-perplexity) of one protein from its [n, 33] table (NaN rows skipped)."""
    wt = log_probs.gather(1, torch.as_tensor(np.asarray(ids), dtype=torch.long)[:, None])[:, 0]
    ok = ~torch.isnan(wt)
    pll = wt[ok].sum()
    return wt, float(pll), float(torch.exp(-pll / max(int(ok.sum()), 1)))


# ------------------------------------------------------------------------------------------------ the fixture's inputs
FIXTURE_LENGTHS = (1, 2, 17, 64)
SCAN_LENGTHS = (9, 17)


def fixture_sequences() -> List[List[str]]:
    """Three variants of one batch of 1, 2, 17 and 64 residues: no mask, one mask per row, several masks in the longer rows."""
    plain = [synth.synth_protein(n, 40 + i) for i, n in enumerate(FIXTURE_LENGTHS)]

    def masked(s, pos):
        return "".join("<mask>" if j in pos else c for j, c in enumerate(s))
    one = [masked(s, {len(s) // 2}) for s in plain]
    several = [masked(s, {0, len(s) // 3, len(s) - 1} | set(range(5, len(s), 11))) for s in plain]
    return [plain, one, several]


def scan_sequences() -> List[str]:
    return [synth.synth_protein(n, 60 + i) for i, n in enumerate(SCAN_LENGTHS)]


def fixture_tokens() -> np.ndarray:
    """int32 [3, 4, 66]: the three variants through the batch converter (<cls> residues <eos>, <pad>)."""
    return np.stack([batch_convert(v)[0] for v in fixture_sequences()])


def ids_of(seq: str) -> np.ndarray:
    return encode_array(seq)
