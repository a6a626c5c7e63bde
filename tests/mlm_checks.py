"""Checks of the ESM-2 masked-LM head that tests/test_gpu_mlm.py and its bf16 child (tests/bf16_mlm_check.py) share: the head's two
launches alone against fp64 on the same operands (opus_debug_esm2_lm_head), the row gather (opus_esm2_lm_head) and the micro
model against the fixture tests/golden/mlm_micro.npz."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth
from opus_pllm_amd.alphabet import batch_convert_packed
import mlm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_ROWS = (1, 2, 63, 64, 65, 257)          # around the 64-row wave / tile edges, more than one workgroup, odd counts
OFFSET_SIGMAS = 30.0                           # |mu| / sigma of the "large common offset" states, as the LN-fusion tests use
V = 33


def enc_cfg(dim: int, heads: int, layers: int = 2, max_batch: int = 8, max_enc_tokens: int = 66):
    return opa.OpusConfig(enc_layers=layers, enc_dim=dim, enc_heads=heads, enc_ffn=4 * dim, proj_dim=256,
                          dec_layers=1, dec_dim=256, dec_heads=4, dec_kv_heads=2, dec_head_dim=64, dec_ffn=512,
                          dec_vocab=512, max_batch=max_batch, max_enc_tokens=max_enc_tokens, max_prompt=64,
                          max_new_tokens=8).validate()


def stream(model) -> int:
    return torch.cuda.current_stream(model.device).cuda_stream


def debug_head(model, hidden: torch.Tensor, log_softmax: bool) -> torch.Tensor:
    """opus_debug_esm2_lm_head on fp32 states [R, De] -> fp32 [R, 33] (NaN-filled first: every element must be written)."""
    R = hidden.shape[0]
    out = torch.full((R, V), float("nan"), dtype=torch.float32, device=model.device)
    _cabi.check(model._lib.opus_debug_esm2_lm_head(model._ctx, hidden.data_ptr(), R, 1 if log_softmax else 0, out.data_ptr(), stream(model)))
    torch.cuda.synchronize(model.device)
    return out


def lm_head(model, rows: Optional[Sequence[int]], R: int, log_softmax: bool = False) -> torch.Tensor:
    """opus_esm2_lm_head on the context's encoder result; rows None: the first R rows in order."""
    out = torch.full((max(R, 1), V), float("nan"), dtype=torch.float32, device=model.device)      # (R = 0: still a real pointer)
    d_rows = None if rows is None else torch.tensor(list(rows), dtype=torch.int32, device=model.device)
    _cabi.check(model._lib.opus_esm2_lm_head(model._ctx, None if d_rows is None else d_rows.data_ptr(), R, 1 if log_softmax else 0,
                                             out.data_ptr(), stream(model)))
    torch.cuda.synchronize(model.device)
    return out[:R]


def encode_packed(model, seqs: Sequence[str]) -> int:
    """One opus_esm2_encode_packed call on the current stream -> the number of token rows it left in the context."""
    toks, cu = batch_convert_packed(seqs)
    B = len(cu) - 1
    d_tok = torch.from_numpy(toks).to(model.device)
    pooled = torch.empty((B, model.cfg.enc_dim), dtype=torch.float32, device=model.device)
    cu_arr = (C.c_int32 * (B + 1))(*[int(v) for v in cu])
    _cabi.check(model._lib.opus_esm2_encode_packed(model._ctx, d_tok.data_ptr(), cu_arr, B, pooled.data_ptr(), stream(model)))
    torch.cuda.synchronize(model.device)
    return int(cu[-1])


def ref_head_fp64(model, cfg, head, hidden: torch.Tensor) -> torch.Tensor:
    """fp64 (torch, on the GPU) on the operands the kernels read: the fp32 states as given and the head's tensors, whose synthetic
    values are exact in the build's operand type."""
    emb = torch.from_numpy(synth.hash_normal(synth.tensor_seed("enc.embed_tokens", 0), 0, V * cfg.enc_dim, 1.0).reshape(V, cfg.enc_dim))
    h = {k: torch.from_numpy(np.ascontiguousarray(v)).to(model.device) for k, v in head.items()}
    return mlm_ref.head_logits(hidden, h, emb.to(model.device), cfg.enc_ln_eps, torch.float64)


def kernel_vs_fp64(model, cfg, head, rows=KERNEL_ROWS, seed: int = 0) -> dict:
    """Every R x {random states, states with a common offset of 30 sigma} x {logits, log-softmax}: the worst figures.
    rel = max |logits - ref| / max |ref|; col32 / last_row: the same over column 32 and over row R - 1 alone; self_abs: the
    log-softmax output against the fp64 log-softmax of the kernel's OWN logits; bitwise: a second launch gives the same bits."""
    o = {"rel": 0.0, "col32": 0.0, "last_row": 0.0, "self_abs": 0.0, "bitwise": True, "finite": True, "cases": 0}
    g = torch.Generator().manual_seed(1000 + seed + cfg.enc_dim)
    for R in rows:
        for offset in (0.0, OFFSET_SIGMAS):
            x = torch.randn(R, cfg.enc_dim, generator=g)
            if offset:
                x = x + offset * torch.where(torch.rand(R, 1, generator=g) < 0.5, -1.0, 1.0)
            x = x.to(model.device)
            ref = ref_head_fp64(model, cfg, head, x)
            scale = float(ref.abs().max())
            lg = debug_head(model, x, False)
            ls = debug_head(model, x, True)
            o["finite"] &= bool(torch.isfinite(lg).all() and torch.isfinite(ls).all())
            err = (lg.double() - ref).abs()
            o["rel"] = max(o["rel"], float(err.max()) / scale)
            o["col32"] = max(o["col32"], float(err[:, 32].max()) / scale)
            o["last_row"] = max(o["last_row"], float(err[R - 1].max()) / scale)
            o["self_abs"] = max(o["self_abs"], float((ls.double() - torch.log_softmax(lg.double(), -1)).abs().max()))
            o["bitwise"] &= torch.equal(lg.view(torch.int32), debug_head(model, x, False).view(torch.int32))
            o["bitwise"] &= torch.equal(ls.view(torch.int32), debug_head(model, x, True).view(torch.int32))
            o["cases"] += 2
    return o


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def gather_checks(model, seqs: Sequence[str]) -> dict:
    """The row lists of opus_esm2_lm_head against the all-rows result of the same encoder call, bit for bit."""
    M = encode_packed(model, seqs)
    full = lm_head(model, None, M)
    o = {"M": M}
    o["arange"] = same_bits(lm_head(model, range(M), M), full)
    o["first_last"] = same_bits(lm_head(model, [0, M - 1], 2), full[[0, M - 1]])
    o["repeat"] = same_bits(lm_head(model, [5, 5, 7, 5], 4), full[[5, 5, 7, 5]])
    desc = list(range(M - 1, -1, -1))
    o["descending"] = same_bits(lm_head(model, desc, M), full[desc])
    o["prefix"] = same_bits(lm_head(model, None, 3), full[:3])
    o["log_softmax_self"] = float((lm_head(model, [7], 1, True).double() - torch.log_softmax(full[7:8].double(), -1)).abs().max())
    return o


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def micro_vs_fixture(model) -> dict:
    """get_residue_logits and the masked scan of the micro model against tests/golden/mlm_micro.npz."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mlm_micro.npz"))
    enc = model.get_protein_encoder()
    o = {"logit_std": float(g["logit_std"]), "logits_rel": 0.0, "mask_rows_rel": 0.0, "shapes_ok": True}
    for v, seqs in enumerate(mlm_ref.fixture_sequences()):
        got = enc.get_residue_logits([(f"p{i}", s) for i, s in enumerate(seqs)])
        refs, gots, mrefs, mgots = [], [], [], []
        for i in range(len(seqs)):
            t = g["tokens"][v, i]
            n = int((t != 1).sum()) - 2
            o["shapes_ok"] &= tuple(got[i].shape) == (n, V)
            ref = torch.from_numpy(g["logits"][v, i, 1:n + 1])
            refs.append(ref); gots.append(got[i].cpu())
            m = torch.from_numpy(t[1:n + 1] == 32)
            mrefs.append(ref[m]); mgots.append(got[i].cpu()[m])
        o["logits_rel"] = max(o["logits_rel"], rel_l2(torch.cat(gots), torch.cat(refs)))
        if v:
            o["mask_rows_rel"] = max(o["mask_rows_rel"], rel_l2(torch.cat(mgots), torch.cat(mrefs)))
    seqs = mlm_ref.scan_sequences()
    res = enc.score_mutations(seqs, mode="masked-marginals")
    o["scan_rel"] = o["wt_rel"] = o["ppl_log_rel"] = 0.0
    for i, s in enumerate(seqs):
        ref = torch.from_numpy(g[f"scan_log_probs_{i}"]).double()
        wt, pll, ppl = mlm_ref.summarize(ref, g[f"scan_tokens_{i}"])
        o["scan_rel"] = max(o["scan_rel"], rel_l2(res.log_probs[i], ref))
        o["wt_rel"] = max(o["wt_rel"], rel_l2(res.wt_log_prob[i], wt))
        o["ppl_log_rel"] = max(o["ppl_log_rel"], abs(float(torch.log(res.pseudo_perplexity[i])) - np.log(ppl)) / abs(np.log(ppl)))
        o["shapes_ok"] &= bool(torch.allclose(res.scores[i], res.log_probs[i] - res.wt_log_prob[i][:, None], equal_nan=True))
        o["shapes_ok"] &= abs(float(res.pseudo_log_likelihood[i]) - float(res.wt_log_prob[i].sum())) < 1e-4
    n = sum(len(s) for s in seqs)
    o["rows_evaluated"], o["encoder_calls"], o["copies"] = res.rows_evaluated, res.encoder_calls, n
    return o
