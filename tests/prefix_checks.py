"""Checks of shared-prefix scoring (OpusLlamaForCausalLM.cache_prefix / score_continuations) shared by tests/test_gpu_prefix.py
and its bf16 child tests/bf16_prefix_check.py: each returns a dict of observations; the callers assert the bounds of their build.
Test infrastructure, not product code."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
import forward_checks as fc

GOLD = fc.GOLD


# ------------------------------------------------------------------------------------------------ the attention kernel alone
KERNEL_SHAPES = [            # (head_dim, heads, kv heads): groups 1, 2, 4, 7 over head dims 16 / 64 / 128
    (16, 4, 4), (16, 8, 4), (64, 4, 2), (64, 7, 1), (128, 8, 2), (128, 14, 2),
]
KERNEL_NS = (1, 5, 16, 17, 64, 130)


def _attn_ref(q, kh, vh, kn, vn, kstart, src, G):
    """fp64: q [R, n, nh, hd], kh / vh [P, nkv, Tp, hd], kn / vn [R, n, nkv, hd] -> [R, n, nh hd]."""
    R, n, nh, hd = q.shape
    Tp = kh.shape[2]
    out = torch.empty((R, n, nh, hd), dtype=torch.float64)
    causal = torch.arange(n)[None, :] <= torch.arange(n)[:, None]                     # [t, t']
    for r in range(R):
        p = int(src[r])
        K = torch.cat([kh[p, :, int(kstart[p]):], kn[r].transpose(0, 1)], 1).repeat_interleave(G, 0)   # [nh, L + n, hd]
        V = torch.cat([vh[p, :, int(kstart[p]):], vn[r].transpose(0, 1)], 1).repeat_interleave(G, 0)
        L = Tp - int(kstart[p])
        s = torch.einsum("thd,hjd->htj", q[r], K) * hd ** -0.5
        vis = torch.cat([torch.ones((n, L), dtype=torch.bool), causal], 1)
        s = s.masked_fill(~vis[None], float("-inf"))
        out[r] = torch.einsum("htj,hjd->thd", torch.softmax(s, -1), V)
    return out.reshape(R, n, nh * hd)


def attn_kernel(dev) -> dict:
    """opus_debug_attn_prefix against fp64: every KERNEL_SHAPES x KERNEL_NS, prefixes up to max_prompt with left-padded rows, a
    row map with repeats in permuted order; the worst absolute error per shape."""
    dt = _cabi.operand_dtype()
    lib = _cabi.lib()
    obs = {}
    for hd, nh, nkv in KERNEL_SHAPES:
        cfg = opa.micro(dec_dim=max(64, nh * hd), dec_heads=nh, dec_kv_heads=nkv, dec_head_dim=hd, max_prompt=160, max_batch=4)
        model = fc.make_model(cfg, dev)
        G = nh // nkv
        worst = 0.0
        for n in KERNEL_NS:
            gen = torch.Generator().manual_seed(hd * 1000 + nh * 10 + n)
            P = 3
            Tp = cfg.max_prompt if n % 2 else 37
            kstart = torch.tensor([0, 5, Tp - 1], dtype=torch.int32)                  # (a row of one real slot)
            src = torch.tensor([2, 0, 0, 1, 2, 2, 0], dtype=torch.int32)             # repeats, permuted order
            R = src.numel()
            QKV = (nh + 2 * nkv) * hd
            qkv = torch.randn(R * n, QKV, generator=gen).to(dt)
            kh = torch.randn(P, nkv, Tp, hd, generator=gen).to(dt)
            vh = torch.randn(P, nkv, Tp, hd, generator=gen).to(dt)
            q = qkv[:, : nh * hd].double().view(R, n, nh, hd)
            kn = qkv[:, nh * hd: (nh + nkv) * hd].double().view(R, n, nkv, hd)
            vn = qkv[:, (nh + nkv) * hd:].double().view(R, n, nkv, hd)
            ref = _attn_ref(q, kh.double(), vh.double(), kn, vn, kstart, src, G)
            d = lambda t: t.contiguous().to(dev)                                       # noqa: E731
            out = torch.zeros(R * n, nh * hd, dtype=dt, device=dev)
            h_src = (C.c_int32 * R)(*src.tolist())
            dq, dk, dv, dks = d(qkv), d(kh), d(vh), d(kstart)
            _cabi.check(lib.opus_debug_attn_prefix(model._ctx, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dks.data_ptr(), P, Tp,
                                                   R, n, h_src, out.data_ptr(), None))
            torch.cuda.synchronize()
            err = float((out.double().cpu().view(R, n, nh * hd) - ref).abs().max())
            worst = max(worst, err)
        obs[f"hd{hd}_g{G}"] = worst
        del model
    return obs


# ------------------------------------------------------------------------------------------------ the reference's forward
def golden_split(dev) -> dict:
    """Rows of tests/golden/forward_micro.npz (the reference's own forward), split at their first counted label: the prompt in
    front of it is the prefix, the rest of the row the continuation.  The continuation's token log-probs against the fixture's,
    with proteins (case a) and without (case c); case b's splice is truncated, d has no labels."""
    cfg = opa.micro()
    model = fc.make_model(cfg, dev)
    g = np.load(os.path.join(GOLD, "forward_micro.npz"))
    seqs = json.load(open(os.path.join(GOLD, "forward_micro.seqs.json")))
    obs = {}
    for tag in "ac":
        ids, mask, lab = g[tag + ".ids"], g[tag + ".mask"].astype(bool), g[tag + ".labels"]
        B = ids.shape[0]
        pre, cont, want = [], [], []
        for b in range(B):
            real = np.flatnonzero(mask[b])
            t0 = int(np.flatnonzero(lab[b] != -100)[0])
            pre.append(ids[b, real[real < t0]])
            tail = real[real >= t0]
            assert (ids[b, tail] >= 0).all()                                        # (no placeholder behind the split)
            cont.append(torch.from_numpy(ids[b, tail].astype(np.int64)))
            counted = lab[b, tail] != -100
            ref_row = g[tag + ".token_logprobs"][b][g[tag + ".labels_out"][b] != -100]
            want.append((counted, ref_row))
        T = max(len(p) for p in pre)
        pids = np.full((B, T), 2, dtype=np.int64)
        pm = np.zeros((B, T), dtype=bool)
        for b, p in enumerate(pre):
            pids[b, T - len(p):] = p
            pm[b, T - len(p):] = True
        kw = dict(seq=seqs) if bool(g[tag + ".has_seq"]) else {}
        prefix = model.cache_prefix(torch.from_numpy(pids), attention_mask=torch.from_numpy(pm), **kw)
        res = model.score_continuations(prefix, cont)
        err = 0.0
        for b, (counted, ref_row) in enumerate(want):
            got = res.token_logprobs[b].double().cpu()[: len(counted)][torch.from_numpy(counted)]
            assert got.numel() == ref_row.size
            err = max(err, float((got - torch.from_numpy(ref_row)).abs().max()))
        obs[tag] = err
    del model
    return obs


# ------------------------------------------------------------------------------------------------ forward() on the concatenation
def _prefix_batch(cfg, P, K, seed, lp=(14, 30), lc=(1, 8)):
    """P left-padded prompts and K ragged continuations per prompt (rows p K .. p K + K - 1)."""
    rng = np.random.default_rng(seed)
    prompts = [rng.integers(3, cfg.dec_vocab, int(rng.integers(lp[0], lp[1] + 1))) for _ in range(P)]
    conts = [rng.integers(3, cfg.dec_vocab, int(rng.integers(lc[0], lc[1] + 1))) for _ in range(P * K)]
    conts[0] = rng.integers(3, cfg.dec_vocab, lc[1])                                   # (one of the longest length)
    T = max(len(p) for p in prompts)
    ids = torch.full((P, T), 2, dtype=torch.long)
    mask = torch.zeros((P, T), dtype=torch.bool)
    for b, p in enumerate(prompts):
        ids[b, T - len(p):] = torch.from_numpy(p)
        mask[b, T - len(p):] = True
    return prompts, conts, ids, mask


def _concat(cfg, prompts, conts, src):
    """Right-padded concatenations prompt + continuation with labels on the continuation."""
    rows = [np.concatenate([prompts[int(p)], c]) for p, c in zip(src, conts)]
    T = max(len(r) for r in rows)
    R = len(rows)
    ids = torch.full((R, T), 2, dtype=torch.long)
    mask = torch.zeros((R, T), dtype=torch.bool)
    labels = torch.full((R, T), -100, dtype=torch.long)
    for r, (row, c) in enumerate(zip(rows, conts)):
        ids[r, : len(row)] = torch.from_numpy(row)
        mask[r, : len(row)] = True
        labels[r, len(row) - len(c): len(row)] = torch.from_numpy(c)
    return ids, mask, labels


def vs_forward(dev, cfg, P, K, seed=0, oracle_check=True) -> dict:
    """R = P K > max_batch ragged continuations (K per prompt, repeated prefix rows, rows shuffled) against forward(labels) on the
    concatenated rows and against the fp32 oracle on the same rows; scoring twice bitwise equal."""
    model = fc.make_model(cfg, dev)
    prompts, conts, ids, mask = _prefix_batch(cfg, P, K, seed)
    perm = np.random.default_rng(seed + 1).permutation(P * K)
    src = np.repeat(np.arange(P), K)[perm]
    conts = [conts[i] for i in perm]
    prefix = model.cache_prefix(ids, attention_mask=mask)
    res = model.score_continuations(prefix, [torch.from_numpy(c) for c in conts], prefix_rows=torch.from_numpy(src))
    res2 = model.score_continuations(prefix, [torch.from_numpy(c) for c in conts], prefix_rows=torch.from_numpy(src))
    cids, cmask, clab = _concat(cfg, prompts, conts, src)
    fwd = model(cids, attention_mask=cmask, labels=clab, return_logits=False)
    got = res.token_logprobs.double().cpu()
    # forward's token_logprobs sit at the label positions: the continuation of row r starts at len(prompt)
    want = torch.zeros_like(got)
    for r, c in enumerate(conts):
        a = len(prompts[int(src[r])])
        want[r, : len(c)] = fwd.token_logprobs[r, a: a + len(c)].double().cpu()
    lens = torch.tensor([len(c) for c in conts])
    valid = torch.arange(got.shape[1])[None, :] < lens[:, None]
    obs = dict(
        R=len(conts), max_batch=cfg.max_batch,
        fwd_abs=float((got - want)[valid].abs().max()),
        zero_pad=bool((got[~valid] == 0).all()),
        bitwise=bool(torch.equal(res.token_logprobs, res2.token_logprobs)),
        sums_ok=bool(torch.allclose(res.logprob.cpu(), res.token_logprobs.sum(1).cpu())),
        n_tokens_ok=bool(torch.equal(res.n_tokens.cpu(), lens)),
    )
    if oracle_check:
        import oracle
        W = fc.Canon32(cfg, dev)
        emb = W["dec.embed_tokens"][cids]
        f = oracle.opt_forward if cfg.dec_arch == 1 else oracle.llama_forward
        with torch.no_grad():
            ref_logits, _ = f(emb, cmask, W, cfg, all_logits=True)
        _, ref_lp, _ = fc._ref_token_logprobs(ref_logits, clab)
        want_o = torch.zeros_like(got)
        for r, c in enumerate(conts):
            a = len(prompts[int(src[r])])
            want_o[r, : len(c)] = ref_lp[r, a: a + len(c)]
        obs["oracle_abs"] = float((got - want_o)[valid].abs().max())
    del model
    return obs
