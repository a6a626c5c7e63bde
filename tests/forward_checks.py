"""Checks of OpusLlamaForCausalLM.forward (teacher-forced loss / token log-probs / logits) shared by tests/test_gpu_forward.py and
its bf16 child tests/bf16_forward_check.py: each returns a dict of observations; the callers assert the bounds of their build.
Test infrastructure, not product code."""
from __future__ import annotations

import json
import os
from collections.abc import Mapping

import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth
from opus_pllm_amd.model import OpusLlamaForCausalLM
from opus_pllm_amd.weights import DeviceWeights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN_TAU = 0.05


def make_model(cfg, dev):
    return OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)


def rel_l2(a, b) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class Canon32(Mapping):
    """The canonical (reference-named) tensors of the synthetic model as fp32 host tensors, generated on the GPU by
    opus_fill_synth straight into fp32 - the values the device weights hold in either operand dtype (the generator rounds to
    the build's 16-bit type) - on first use, a bounded number kept."""

    def __init__(self, cfg, dev, keep_bytes: float = 14e9):
        self.cfg, self.dev, self.keep = cfg, torch.device(dev), keep_bytes
        self.spec = {n: (sh, std, mean) for n, sh, std, mean in synth.canonical_spec(cfg)}
        self._cache, self._bytes = {}, 0

    def __iter__(self):
        return iter(self.spec)

    def __len__(self):
        return len(self.spec)

    def __getitem__(self, name):
        if name in self._cache:
            return self._cache[name]
        shape, std, mean = self.spec[name]
        rows = int(shape[0])
        cols = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        t = torch.empty(shape, dtype=torch.float32, device=self.dev)
        _cabi.check(_cabi.lib().opus_fill_synth(t.data_ptr(), _cabi.OPUS_F32, rows, cols, synth.tensor_seed(name, 0), std, mean,
                                                rows, rows, 0, 0, 0, 0.0, 0.0, torch.cuda.current_stream(self.dev).cuda_stream))
        host = t.cpu()
        del t
        while self._cache and self._bytes + host.numel() * 4 > self.keep:
            old = self._cache.pop(next(iter(self._cache)))
            self._bytes -= old.numel() * 4
        self._cache[name] = host
        self._bytes += host.numel() * 4
        return host


def _ref_token_logprobs(logits: torch.Tensor, labels: torch.Tensor):
    """fp64 log p(labels[b, t]) from the logits at t - 1, 0 where not counted; (loss, token log-probs, counted mask)."""
    lp = torch.log_softmax(logits.double(), dim=-1)
    B, T, _ = logits.shape
    out = torch.zeros((B, T), dtype=torch.float64)
    cnt = torch.zeros((B, T), dtype=torch.bool)
    for b in range(B):
        for t in range(1, T):
            y = int(labels[b, t])
            if y != -100:
                out[b, t] = lp[b, t - 1, y]
                cnt[b, t] = True
    return float(-out[cnt].mean()) if cnt.any() else float("nan"), out, cnt


def golden_cases(dev) -> dict:
    """Cases (a)-(d) of tests/golden/forward_micro.npz (the reference's own forward, tools/gen_golden_forward.py)."""
    cfg = opa.micro()
    model = make_model(cfg, dev)
    g = np.load(os.path.join(GOLD, "forward_micro.npz"))
    seqs = json.load(open(os.path.join(GOLD, "forward_micro.seqs.json")))
    obs = {}
    for tag in "abcd":
        ids = torch.from_numpy(g[tag + ".ids"])
        mask = torch.from_numpy(g[tag + ".mask"])
        labels = torch.from_numpy(g[tag + ".labels"]) if g[tag + ".labels"].size else None
        ml = int(g[tag + ".max_length"])
        if ml >= 0:
            model.config.tokenizer_model_max_length = ml
        kw = dict(seq=seqs) if bool(g[tag + ".has_seq"]) else {}
        out = model(ids, attention_mask=mask, labels=labels, **kw)
        if ml >= 0:
            del model.config.tokenizer_model_max_length
        ref = torch.from_numpy(g[tag + ".logits"])
        valid = torch.from_numpy(g[tag + ".mask_out"]).bool()
        got = out.logits.float().cpu()
        o = dict(shape_ok=tuple(got.shape) == tuple(ref.shape))
        if o["shape_ok"]:
            o["logits_rel_l2"] = rel_l2(got[valid], ref[valid])
            r = ref[valid]
            top2 = r.topk(2, dim=-1).values
            dec = (top2[:, 0] - top2[:, 1]) > MARGIN_TAU
            o["argmax_bad"] = int((got[valid].argmax(-1) != r.argmax(-1))[dec].sum())
            o["argmax_checked"] = int(dec.sum())
        if labels is None:
            o["loss_is_none"] = out.loss is None
        else:
            ref_loss = float(g[tag + ".loss"])
            o["loss_rel"] = abs(float(out.loss) - ref_loss) / abs(ref_loss)
            o["lp_abs"] = float((out.token_logprobs.double().cpu() - torch.from_numpy(g[tag + ".token_logprobs"])).abs().max())
            o["n_tokens_ok"] = out.n_tokens == int(g[tag + ".n_tokens"])
        obs[tag] = o
    del model
    return obs


def xent_kernel(dev) -> dict:
    """opus_debug_xent against fp64 log_softmax: flat, peaked, spread and large-magnitude rows, an ignored target, a row block
    that does not start on a 16-byte boundary; two calls bitwise equal."""
    dt = _cabi.operand_dtype()
    model = make_model(opa.micro(), dev)
    lib = _cabi.lib()
    gen = torch.Generator().manual_seed(0)
    obs = dict(lp_abs=0.0, lse_excess=0.0, bitwise=True, ignored_zero=True)
    s = torch.cuda.current_stream(dev).cuda_stream
    for V in (97, 50272, 128256, 151936):
        rows = [torch.zeros(V), torch.randn(V, generator=gen), torch.randn(V, generator=gen) * 4.0,
                (torch.rand(V, generator=gen) * 2 - 1) * 60000.0, (torch.rand(V, generator=gen) * 2 - 1) * 200.0]
        rows[1][V // 3] = 30.0                                               # peaked
        rows[3][V - 2] = 65000.0
        L = torch.stack(rows).to(dt)
        R = L.shape[0]
        tg = torch.tensor([0, V // 3, V - 1, V - 2, -1], dtype=torch.int32)
        Ld = L.double()
        lse_ref = torch.logsumexp(Ld, dim=-1)
        lp_ref = torch.where(tg >= 0, Ld[torch.arange(R), tg.clamp(min=0).long()] - lse_ref, torch.zeros(R, dtype=torch.float64))
        for off in (0, 1):
            buf = torch.zeros(R * V + off, dtype=dt, device=dev)
            buf[off:] = L.reshape(-1).to(dev)
            d_tg = tg.to(dev)
            res = []
            for _ in range(2):
                lp = torch.full((R,), 7.0, device=dev)
                lse = torch.full((R,), 7.0, device=dev)
                _cabi.check(lib.opus_debug_xent(model._ctx, buf.data_ptr() + off * buf.element_size(), R, V, d_tg.data_ptr(),
                                                lp.data_ptr(), lse.data_ptr(), s))
                res.append((lp.cpu(), lse.cpu()))
            obs["bitwise"] &= torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
            lp, lse = res[0]
            obs["lp_abs"] = max(obs["lp_abs"], float((lp.double() - lp_ref).abs().max()))
            # lse is an fp32 number: at |lse| ~ 6.5e4 its own rounding is 2e-3, so the bound is 1e-4 + 2^-23 |lse|
            obs["lse_excess"] = max(obs["lse_excess"], float(((lse.double() - lse_ref).abs() - 2.0 ** -23 * lse_ref.abs()).max()))
            obs["ignored_zero"] &= float(lp[4]) == 0.0
    del model
    return obs


def _text_batch(cfg, B, T, seed):
    """Right-padded text rows of different lengths; labels = the last `ans` valid ids of a row, -100 elsewhere."""
    rng = np.random.default_rng(seed)
    ids = torch.full((B, T), 2, dtype=torch.long)
    mask = torch.zeros((B, T), dtype=torch.bool)
    labels = torch.full((B, T), -100, dtype=torch.long)
    for b in range(B):
        n = T if b == 0 else int(rng.integers(T // 2, T + 1))
        ids[b, :n] = torch.from_numpy(rng.integers(3, cfg.dec_vocab, n))
        mask[b, :n] = True
        ans = max(2, n // 3)
        labels[b, n - ans:n] = ids[b, n - ans:n]
    return ids, mask, labels


def vs_oracle(dev, cfg, B, T, seed=0) -> dict:
    """forward() on text rows against the fp32 oracle with all_logits=True: token log-probs, loss, logits; the loss-only path
    against the logits path, and the loss-only path run twice."""
    import oracle
    model = make_model(cfg, dev)
    W = Canon32(cfg, dev)
    ids, mask, labels = _text_batch(cfg, B, T, seed)
    emb = W["dec.embed_tokens"][ids]
    fwd = oracle.opt_forward if cfg.dec_arch == 1 else oracle.llama_forward
    with torch.no_grad():
        ref_logits, _ = fwd(emb, mask, W, cfg, all_logits=True)
    ref_loss, ref_lp, cnt = _ref_token_logprobs(ref_logits, labels)
    full = model(ids, attention_mask=mask, labels=labels)
    lo1 = model(ids, attention_mask=mask, labels=labels, return_logits=False)
    lo2 = model(ids, attention_mask=mask, labels=labels, return_logits=False)
    got = full.logits.float().cpu()
    obs = dict(
        lp_abs=float((full.token_logprobs.double().cpu() - ref_lp)[cnt].abs().max()),
        lossonly_lp_abs=float((lo1.token_logprobs.double().cpu() - ref_lp)[cnt].abs().max()),
        loss_rel=abs(float(full.loss) - ref_loss) / abs(ref_loss),
        lossonly_loss_rel=abs(float(lo1.loss) - ref_loss) / abs(ref_loss),
        logits_rel_l2=rel_l2(got[mask], ref_logits[mask]),
        logit_absmax=float(ref_logits[mask].abs().max()),
        paths_abs=float((lo1.token_logprobs - full.token_logprobs).abs().max()),
        lossonly_bitwise=bool(torch.equal(lo1.token_logprobs, lo2.token_logprobs) and torch.equal(lo1.loss, lo2.loss)),
        zero_elsewhere=bool((full.token_logprobs.cpu()[~cnt] == 0).all() and (lo1.token_logprobs.cpu()[~cnt] == 0).all()),
        n_tokens_ok=full.n_tokens == lo1.n_tokens == int(cnt.sum()),
        logits_none=lo1.logits is None,
    )
    del model
    return obs
