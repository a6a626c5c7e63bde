"""Checks of generate(prefix=...) and the prefill behind a detached prefix, shared by tests/test_gpu_prefix_generate.py: each
returns a dict of observations; the caller asserts the bounds.  The plain path - generate() / prefill_logits() on the
concatenated prompts - is the reference everywhere.  Test infrastructure, not product code."""
from __future__ import annotations

import copy

import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.model import OpusPrefix, _BehindCall
from opus_pllm_amd.prefix import plan_prefill_behind

import forward_checks as fc
from gpu_helpers import rel_l2

PAD = 2
MARGIN_TAU = 0.05


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bitwise (NaN-proof)"""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape:
        return False
    w = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.view(w), b.view(w)))


def left_pad(rows, width=None):
    width = max(len(r) for r in rows) if width is None else width
    ids = torch.full((len(rows), width), PAD, dtype=torch.long)
    mask = torch.zeros((len(rows), width), dtype=torch.bool)
    for i, r in enumerate(rows):
        ids[i, width - len(r):] = torch.as_tensor(np.asarray(r), dtype=torch.long)
        mask[i, width - len(r):] = True
    return ids, mask


def right_pad(rows):
    width = max(len(r) for r in rows)
    ids = torch.zeros((len(rows), width), dtype=torch.long)
    mask = torch.zeros((len(rows), width), dtype=torch.bool)
    for i, r in enumerate(rows):
        ids[i, : len(r)] = torch.as_tensor(np.asarray(r), dtype=torch.long)
        mask[i, : len(r)] = True
    return ids, mask


def text_batch(cfg, plens, slens, src, seed):
    """Text-only prompts: prefixes of plens[p] ids, suffixes of slens[r] ids, row r behind prefix src[r]; (prefixes, suffixes,
    concatenations), lists of int arrays.  Pure NumPy, so that seeds can be chosen on the CPU oracle."""
    rng = np.random.default_rng(seed)
    pre = [rng.integers(3, cfg.dec_vocab, int(n)) for n in plens]
    suf = [rng.integers(3, cfg.dec_vocab, int(n)) for n in slens]
    cat = [np.concatenate([pre[int(p)], s]) for p, s in zip(src, suf)]
    return pre, suf, cat


def embed(model, ids, mask, left: bool):
    """Token embeddings of text-only rows through the splice: left-padded as generate() prefills them, or right-padded as the
    suffix rows of a prefill behind a prefix."""
    cfg = model.cfg
    dummy = torch.zeros((ids.shape[0], cfg.n_prot_tokens, cfg.dec_dim), dtype=_cabi.operand_dtype(), device=model.device)
    emb, m, _ = model._splice(ids, mask, dummy, left)
    return emb, m


def live_copy_detached(prefix: OpusPrefix) -> OpusPrefix:
    """A detached twin of a live handle that leaves the live one live (detach() converts in place)."""
    return copy.copy(prefix).detach()


# ------------------------------------------------------------------------------------------------ placement, bit for bit
PLACE_SHAPES = [(16, 4, 4), (64, 4, 2), (128, 2, 1)]          # (head_dim, heads, kv heads): kv heads 4 / 2 / 1
PLACE_LP = (1, 31, 32, 33)                                      # real prefix tokens of the four prefix rows
PLACE_N = 34
PLACE_LENS = (34, 33, 3, 1, 34, 17, 2)                          # d_r = 0, 1, 31, 33, 0, 17, 32
PLACE_MAPS = ([2, 0, 0, 1, 2, 2, 0], [3, 1, 3, 0, 2, 1, 3])     # repeats in permuted order; the first leaves prefix row 3 unused
PLACE_TP = (33, 96)                                             # T' = 67 crosses 64, T' = 130 crosses 128


def placement(dev, hd, nh, nkv) -> dict:
    """A plain prefill of max_batch rows x T' slots is the sentinel; the prefill behind the prefix must leave rows >= R and the
    slots below kstart' as the sentinel wrote them, and the prefix block of every decode row bit-equal to its snapshot row."""
    cfg = opa.micro(dec_dim=max(64, nh * hd), dec_heads=nh, dec_kv_heads=nkv, dec_head_dim=hd, max_prompt=160, max_batch=8)
    model = fc.make_model(cfg, dev)
    obs = {}
    for Tp in PLACE_TP:
        for mi, src in enumerate(PLACE_MAPS):
            R, n, T = len(src), PLACE_N, Tp + PLACE_N
            # (the splice is as wide as its longest row: a fifth, full-width prefix row - unused by both maps - makes Tp = 96)
            plens = PLACE_LP + ((Tp,) if Tp > max(PLACE_LP) else ())
            pre, suf, _ = text_batch(cfg, plens, PLACE_LENS, src, seed=hd + Tp + mi)
            pids, pmask = left_pad(pre, Tp)
            prefix = model.cache_prefix(pids, attention_mask=pmask, detach=True)
            kst = prefix._kstart.cpu().numpy()
            assert prefix.slots == Tp and kst.tolist() == [Tp - l for l in plens], (Tp, prefix.slots, kst)
            sent_rows = [np.random.default_rng(900 + b).integers(3, cfg.dec_vocab, T - b) for b in range(cfg.max_batch)]
            sids, smask = left_pad(sent_rows, T)
            sent = model.cache_prefix(sids, attention_mask=smask)
            sk, sv, _ = model.export_cache(sent._epoch, cfg.max_batch, T)
            emb, _ = embed(model, *right_pad(suf), left=False)
            _, epoch = model.prefill_logits_behind(prefix, emb, PLACE_LENS, src)
            k, v, nks = model.export_cache(epoch, cfg.max_batch, T)
            nks = nks.cpu().numpy()
            # the geometry is read off prefix.plan_prefill_behind - what generate(prefix=...) plans with and the host test checks
            # against the brute-force restatement - so the tables the kernels consumed are held to the same numbers
            plan = plan_prefill_behind(kst, Tp, src, PLACE_LENS, n, cfg.max_batch, cfg.max_prompt, cfg.max_batch * cfg.max_prompt)
            ok_block = ok_sent = ok_ks = True
            for r in range(cfg.max_batch):
                if r >= R:
                    ok_sent &= same(k[:, r], sk[:, r]) and same(v[:, r], sv[:, r])
                    continue
                p, d = src[r], int(plan.pad[r])
                lp, a = int(plan.prefix_len[r]), int(plan.prefix_slot0[r])
                ok_ks &= int(nks[r]) == int(plan.new_kstart[r]) == kst[p] + d and int(plan.suffix_slot0[r]) == Tp + d
                ok_block &= same(k[:, r, :, a: a + lp], prefix._k[:, p, :, kst[p]:]) and same(v[:, r, :, a: a + lp], prefix._v[:, p, :, kst[p]:])
                ok_sent &= same(k[:, r, :, :a], sk[:, r, :, :a]) and same(v[:, r, :, :a], sv[:, r, :, :a])
                # (the suffix slots are new values: they differ from the sentinel's)
                ok_block &= not same(k[:, r, :, Tp + d:], sk[:, r, :, Tp + d:])
            obs[f"Tp{Tp}_map{mi}"] = dict(block=bool(ok_block), sentinel=bool(ok_sent), kstart=bool(ok_ks))
    del model
    return obs


# ------------------------------------------------------------------------------------------------ logits and K / V vs the plain path
def logits_vs_plain(model, plens, slens, src, seed, steps=4) -> dict:
    """Prefill + `steps` greedy decode steps behind the prefix against the plain prefill of the concatenation, fed the plain
    run's tokens: rel-L2 per step; and layer 0's K / V at the suffix slots against the plain prefill's."""
    cfg = model.cfg
    pre, suf, cat = text_batch(cfg, plens, slens, src, seed)
    R, Tp, n = len(src), max(plens), max(slens)
    cids, cmask = left_pad(cat)
    cemb, cm = embed(model, cids, cmask, left=True)
    plain = [model.prefill_logits(cemb, cm).clone()]
    toks = []
    for _ in range(steps):
        toks.append(plain[-1].argmax(dim=1))
        plain.append(model.decode_logits(toks[-1]).clone())
    ref_pre = model.cache_prefix(cids, attention_mask=cmask)           # (the same prefill again: its epoch reads the cache back)
    Tc = int(cids.shape[1])
    pk, pv, pks = model.export_cache(ref_pre._epoch, R, Tc)
    pids, pmask = left_pad(pre, Tp)
    prefix = model.cache_prefix(pids, attention_mask=pmask, detach=True)
    emb, _ = embed(model, *right_pad(suf), left=False)
    lg, epoch = model.prefill_logits_behind(prefix, emb, slens, src)
    got = [lg.clone()]
    k, v, _ = model.export_cache(epoch, R, Tp + n)
    for t in toks:
        got.append(model.decode_logits(t).clone())
    rel = [rel_l2(g, p) for g, p in zip(got, plain)]
    kv = 0.0
    for r in range(R):
        lp, nr = len(pre[src[r]]), len(suf[r])
        a = int(pks[r]) + lp
        for x, y in ((k, pk), (v, pv)):
            ref = y[0, r, :, a: a + nr].float()
            kv = max(kv, float((x[0, r, :, Tp + n - nr: Tp + n].float() - ref).abs().max() / ref.abs().max()))
    argmax_same = float(np.mean([bool((g.argmax(1) == p.argmax(1)).all()) for g, p in zip(got, plain)]))
    return dict(rel_l2=rel, kv_layer0=kv, T_new=Tp + n, last_slot=Tp + n + steps - 1, argmax_same=argmax_same)


# ------------------------------------------------------------------------------------------------ generate() behind a prefix vs plain
def decisive_compare(got: torch.Tensor, ref: torch.Tensor, logits) -> dict:
    """Ids behind the prefix against the plain run's, up to (excluding) each row's first step whose top-1 margin in the PLAIN
    run's logits (with processors or a constraint on: its processed scores, what the choice is made on) is below MARGIN_TAU;
    the share of decisive steps."""
    got, ref = got.cpu(), ref.cpu()
    R, N = ref.shape
    marg = torch.stack([torch.topk(l.float().cpu(), 2, dim=1).values for l in logits[:N]], 1)       # [R, N, 2]
    marg = marg[..., 0] - marg[..., 1]
    checked, ok = 0, got.shape == ref.shape
    for r in range(R):
        low = (marg[r] < MARGIN_TAU).nonzero()
        m = int(low[0]) if len(low) else N
        ok = ok and bool(torch.equal(got[r, :m], ref[r, :m]))
        checked += m
    return dict(decisive=checked / max(R * N, 1), ids_equal=bool(ok))


def gen_pair(model, plens, slens, src, data_seed, max_new=8, **kw):
    """(plain output with logits, output behind the prefix, prefix, suffix rows) of one generate() each on the same prompts."""
    cfg = model.cfg
    pre, suf, cat = text_batch(cfg, plens, slens, src, data_seed)
    cids, cmask = left_pad(cat)
    base = dict(pad_token_id=PAD, max_new_tokens=max_new, return_dict_in_generate=True, output_logits=True, output_scores=True,
                output_token_logprobs=True)
    base.update(kw)
    plain = model.generate(cids, attention_mask=cmask, **base)
    pids, pmask = left_pad(pre)
    prefix = model.cache_prefix(pids, attention_mask=pmask, detach=True)
    sids, smask = left_pad(suf)
    behind = model.generate(sids, attention_mask=smask, prefix=prefix, prefix_rows=torch.tensor(src), **base)
    return plain, behind, prefix, suf


def draws_follow_fp64_rule(o, mode, seed) -> dict:
    """Every sampled id against the fp64 rule on that step's returned logits with the draw of (seed, row, step)."""
    import oracle.sampling as osamp
    seq, cnt = o.sequences.cpu().numpy(), o.n_tokens.cpu().numpy()
    n = nd = mism = bad = 0
    for t in range(seq.shape[1]):
        lg = o.logits[t].float().cpu().numpy()
        for r in range(seq.shape[0]):
            if t >= cnt[r]:
                continue
            ref = osamp.HeadRef(lg[r], mode["temperature"], mode["top_p"], mode["top_k"])
            pick, dec, lo, hi = ref.draw(np.array([osamp.draw_uniform(seed, r, t)[1]]))
            g = int(seq[r, t])
            n += 1
            nd += int(not dec[0])
            mism += int(dec[0] and g != int(pick[0]))
            bad += int(not ref.admissible(g, int(lo[0]), int(hi[0])))
    return dict(draws=n, nondecisive=nd / max(n, 1), mismatches=mism, inadmissible=bad)


# ------------------------------------------------------------------------------------------------ the fixtures' rows, cut three ways
def cut_rows(ids: np.ndarray, mask: np.ndarray, how: str):
    """Every row of a fixture (ids with one -200 placeholder) cut (i) just behind the placeholder, (ii) just in front of it,
    (iii) before its last token: (prefix rows, suffix rows) as lists of int arrays."""
    pre, suf = [], []
    for b in range(ids.shape[0]):
        row = ids[b][mask[b].astype(bool)]
        at = int(np.flatnonzero(row == -200)[0])
        c = {"behind_seq": at + 1, "before_seq": at, "last_token": len(row) - 1}[how]
        assert 0 < c < len(row)
        pre.append(row[:c])
        suf.append(row[c:])
    return pre, suf


def cut_embeds(emb: torch.Tensor, mask: torch.Tensor, ids: np.ndarray, imask: np.ndarray, n_prot: int, how: str):
    """The same cuts on spliced, left-padded embeddings [B, T, H] (the placeholder is n_prot rows wide there): left-padded prefix
    embeddings + mask, right-padded suffix embeddings + lengths."""
    B, T, H = emb.shape
    cuts = []
    for b in range(B):
        row = ids[b][imask[b].astype(bool)]
        at = int(np.flatnonzero(row == -200)[0])
        L = int(mask[b].sum())
        cuts.append({"behind_seq": at + n_prot, "before_seq": at, "last_token": L - 1}[how])
    Tp = max(cuts)
    n = max(int(mask[b].sum()) - cuts[b] for b in range(B))
    pe, pm = torch.zeros((B, Tp, H), dtype=emb.dtype), torch.zeros((B, Tp), dtype=torch.bool)
    se, lens = torch.zeros((B, n, H), dtype=emb.dtype), []
    for b in range(B):
        real = emb[b][mask[b].bool()]
        c = cuts[b]
        pe[b, Tp - c:], pm[b, Tp - c:] = real[:c], True
        se[b, : real.shape[0] - c] = real[c:]
        lens.append(real.shape[0] - c)
    return pe, pm, se, lens


def prefix_from_embeds(model, emb: torch.Tensor, mask: torch.Tensor) -> OpusPrefix:
    """cache_prefix() for rows that are already embeddings (the family fixtures): opus_llama_prefix + detach."""
    import ctypes as C
    B, T, H = emb.shape
    e = emb.to(model.device, _cabi.operand_dtype()).contiguous()
    m = mask.to(model.device).to(torch.uint8).contiguous()
    s = model._enter()
    with torch.cuda.stream(model._stream):
        last = torch.empty((B, H), dtype=torch.float32, device=model.device)
        epoch = C.c_int64(0)
        _cabi.check(model._lib.opus_llama_prefix(model._ctx, e.data_ptr(), m.data_ptr(), B, T, None, last.data_ptr(), C.byref(epoch), s))
    model._leave()
    return OpusPrefix(model, epoch.value, last, m.sum(dim=1).cpu(), slots=T).detach()


def greedy_behind_embeds(model, prefix, se, lens, max_new, eos=(), pad=PAD):
    call = _BehindCall(prefix, np.asarray(lens), np.arange(len(lens)))
    return model._greedy(se.to(model.device, _cabi.operand_dtype()), None, max_new, list(eos), pad, behind=call)
