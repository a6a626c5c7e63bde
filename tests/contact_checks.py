"""Test infrastructure for ESM-2 contact maps (get_amino_acid_embeddings(return_contacts=True)): reference maps and the checks
that tests/test_gpu_contacts.py and its bf16 child (tests/bf16_contacts_check.py) share.

Two reference forms of EsmContactPredictionHead:
  * `hf_contacts`: transformers' own head class over a full [B, L, H, T, T] attention stack, padding zeroed as
    EsmModel.predict_contacts does;
  * `Reform`: the rank-1 reformulation the kernels use (csrc/contact.hip), fed one layer at a time in fp64, so that a
    33-layer stack never exists.  tests/test_contacts_host.py proves the two equal.
Per-layer attention probabilities are rebuilt from the residual stream the fp32 oracle taps after every layer
(oracle.esm2.esm2_hidden(taps=...)): layer l's input is taps[l - 1] (the scaled embedding for l = 0).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from opus_pllm_amd import _cabi, synth


def hf_contacts(tokens: torch.Tensor, attn: torch.Tensor, weight, bias, pad_idx: int = 1, eos_idx: int = 2) -> torch.Tensor:
    """tokens [B, T] (padded with pad_idx), attn [B, L, H, T, T] -> transformers' EsmContactPredictionHead output [B, T-2, T-2]."""
    from transformers.models.esm.modeling_esm import EsmContactPredictionHead
    B, L, H, T, _ = attn.shape
    head = EsmContactPredictionHead(L * H, bias=True, eos_idx=eos_idx).double()
    with torch.no_grad():
        head.regression.weight.copy_(torch.as_tensor(np.asarray(weight), dtype=torch.float64).reshape(1, -1))
        head.regression.bias.copy_(torch.as_tensor(np.asarray(bias), dtype=torch.float64).reshape(1))
        m = (tokens != pad_idx).to(torch.float64)
        a = attn.double() * m[:, None, None, None, :] * m[:, None, None, :, None]      # predict_contacts' padding zeroing
        return head(tokens, a)


class Reform:
    """logit = bias + A + A^T - sum_c (w_c / s_c) a_c a_c^T over the interior positions of ONE protein (fp64)."""

    def __init__(self, n: int, weight, bias):
        self.n = n
        self.w = torch.as_tensor(np.asarray(weight), dtype=torch.float64).reshape(-1)
        self.bias = float(np.asarray(bias).reshape(-1)[0])
        self.A = torch.zeros(n, n, dtype=torch.float64)
        self.vecs: List[torch.Tensor] = []
        self.c = 0

    def add_layer(self, probs: torch.Tensor) -> None:
        """probs [H, T, T] of this protein (softmax over all T = n + 2 keys)."""
        P = probs.double()[:, 1:self.n + 1, 1:self.n + 1]
        H = P.shape[0]
        w = self.w[self.c:self.c + H]
        self.A += torch.einsum("h,hij->ij", w, P)
        self.vecs.append(P.sum(2) + P.sum(1))                    # a_c [H, n]
        self.c += H

    def logits(self) -> torch.Tensor:
        a = torch.cat(self.vecs, 0)                              # [C, n]
        s = a.sum(1)
        corr = torch.einsum("c,ci,cj->ij", self.w / s, a, a)
        return self.bias + self.A + self.A.T - corr

    def contacts(self) -> torch.Tensor:
        return torch.sigmoid(self.logits())


def layer_probs(x_in: torch.Tensor, W, cfg, l: int) -> torch.Tensor:
    """The fp32 oracle's attention probabilities of layer l for an unpadded [1, T, D] input: [H, T, T]."""
    from oracle.esm2 import _rotary
    D, nh = cfg.enc_dim, cfg.enc_heads
    hd = D // nh
    T = x_in.shape[1]
    p = f"enc.layers.{l}."
    h = F.layer_norm(x_in, (D,), W[p + "ln1.weight"], W[p + "ln1.bias"], cfg.enc_ln_eps)
    q = F.linear(h, W[p + "q.weight"], W[p + "q.bias"]) * hd ** -0.5
    k = F.linear(h, W[p + "k.weight"], W[p + "k.bias"])
    q = _rotary(q.view(1, T, nh, hd).transpose(1, 2), cfg.enc_rope_theta)
    k = _rotary(k.view(1, T, nh, hd).transpose(1, 2), cfg.enc_rope_theta)
    return torch.softmax(q @ k.transpose(-1, -2), dim=-1)[0]


def oracle_protein(seq: str, W, cfg, head) -> dict:
    """One protein through the fp32 oracle: last hidden state rows 1 .. n and the reference contact map (fp64 reformulation)."""
    from oracle.esm2 import esm2_batch_tokens, esm2_hidden
    toks, _ = esm2_batch_tokens([seq])
    taps: List[torch.Tensor] = []
    with torch.no_grad():
        hid = esm2_hidden(toks, W, cfg, taps=taps)
        n = toks.shape[1] - 2
        x0 = W["enc.embed_tokens"][toks] * (1 - 0.15 * 0.8)           # token dropout scale, no <mask> tokens
        rf = Reform(n, head["enc.contact.weight"], head["enc.contact.bias"])
        for l in range(cfg.enc_layers):
            rf.add_layer(layer_probs(x0 if l == 0 else taps[l - 1], W, cfg, l))
    lg = rf.logits()
    return {"hidden": hid[0, 1:n + 1].float(), "logits": lg, "contacts": torch.sigmoid(lg)}


# ------------------------------------------------------------------------------------------------ kernel alone
def debug_contacts(dev, q: torch.Tensor, k: torch.Tensor, cu: Sequence[int], heads: int, hd: int, w: torch.Tensor, ctx=None):
    """opus_debug_contacts on packed rows q / k [M, heads hd] -> (A [sum n^2], rows [sum n, heads], cols [sum n, heads])."""
    lib = _cabi.lib()
    B = len(cu) - 1
    n = [cu[b + 1] - cu[b] - 2 for b in range(B)]
    A = torch.full((max(1, sum(x * x for x in n)),), float("nan"), dtype=torch.float32, device=dev)
    rows = torch.full((max(1, sum(n)), heads), float("nan"), dtype=torch.float32, device=dev)
    cols = torch.full_like(rows, float("nan"))
    need = 256 + 4 * (B + 1) + 4 * heads * sum((x + 63) // 64 * x for x in n) + 256
    scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
    cu_arr = (C.c_int32 * (B + 1))(*cu)
    s = torch.cuda.current_stream(dev).cuda_stream
    _cabi.check(lib.opus_debug_contacts(ctx, q.data_ptr(), k.data_ptr(), q.stride(0), cu_arr, B, heads, hd, w.data_ptr(),
                                        A.data_ptr(), rows.data_ptr(), cols.data_ptr(), scratch.data_ptr(), need, s))
    torch.cuda.synchronize(dev)
    return A, rows, cols


def kernel_vs_fp64(dev, ctx, hd: int, lens=(0, 1, 2, 17, 63, 64, 65, 130, 513, 1024), heads: int = 4, seed: int = 0) -> dict:
    """Packed ragged proteins of n residues each: A, row sums and column sums of the kernel against fp64 on the same operands."""
    g = torch.Generator().manual_seed(seed + hd)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n + 2)
    M = cu[-1]
    q = (torch.randn(M, heads * hd, generator=g) * 2.0 / math.sqrt(hd)).to(_cabi.operand_dtype())
    k = (torch.randn(M, heads * hd, generator=g) * 2.0).to(_cabi.operand_dtype())
    w = torch.randn(heads, generator=g)
    A, rows, cols = debug_contacts(dev, q.to(dev), k.to(dev), cu, heads, hd, w.to(dev), ctx)
    A, rows, cols = A.cpu().double(), rows.cpu().double(), cols.cpu().double()
    qd, kd = q.double(), k.double()
    err = {"A": 0.0, "rows": 0.0, "cols": 0.0}
    ao = vo = 0
    for b, n in enumerate(lens):
        r0, T = cu[b], n + 2
        Q = qd[r0:r0 + T].view(T, heads, hd).transpose(0, 1)
        K = kd[r0:r0 + T].view(T, heads, hd).transpose(0, 1)
        P = torch.softmax(Q @ K.transpose(-1, -2), -1)[:, 1:n + 1, 1:n + 1]
        if n:
            err["A"] = max(err["A"], float((A[ao:ao + n * n].view(n, n) - torch.einsum("h,hij->ij", w.double(), P)).abs().max()))
            err["rows"] = max(err["rows"], float((rows[vo:vo + n] - P.sum(2).T).abs().max()))
            err["cols"] = max(err["cols"], float((cols[vo:vo + n] - P.sum(1).T).abs().max()))
        ao += n * n
        vo += n
    return err


# ------------------------------------------------------------------------------------------------ model level
def model_vs_oracle(model, cfg, seqs: Sequence[str], W, head) -> dict:
    """get_amino_acid_embeddings(return_contacts=True) against the fp32 oracle, protein by protein."""
    embs, maps = model.get_protein_encoder().get_amino_acid_embeddings([(f"p{i}", s) for i, s in enumerate(seqs)], return_contacts=True)
    out = {"contact_abs": 0.0, "emb_rel": 0.0, "logit_std_min": float("inf"), "shapes_ok": True}
    for i, s in enumerate(seqs):
        ref = oracle_protein(s, W, cfg, head)
        n = len(s)
        out["shapes_ok"] &= tuple(embs[i].shape) == (n, cfg.enc_dim) and tuple(maps[i].shape) == (n, n)
        if n == 0:
            continue
        out["contact_abs"] = max(out["contact_abs"], float((maps[i].cpu().double() - ref["contacts"]).abs().max()))
        e = embs[i].cpu().double()
        out["emb_rel"] = max(out["emb_rel"], float((e - ref["hidden"].double()).norm() / ref["hidden"].double().norm()))
        if n > 1:
            out["logit_std_min"] = min(out["logit_std_min"], float(ref["logits"].std()))
    return out


def head_of(cfg, seed: int = 0) -> dict:
    return synth.contact_head(cfg, seed)
