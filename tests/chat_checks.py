"""Checks of generate(return_prefix=True), opus_llama_prefix_export_rows, cache_prefix(prefix=) and ChatSession, shared by
tests/test_gpu_chat.py and its bf16 child tests/bf16_chat_check.py: each returns a dict of observations; the callers assert the
bounds of their build.  Every generated answer is FORCED - a one-member TokenTrie per row, ending in the EOS id - so that no
near-tie decides an id: the ragged row ends are chosen, the raw logits stay raw.  Test infrastructure, not product code."""
from __future__ import annotations

import numpy as np
import torch

from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TokenTrie
from opus_pllm_amd.model import counted_tokens
from opus_pllm_amd.prefix import plan_export_rows

import prefix_generate_checks as pg

EOS, PAD = 1, 2
MAX_NEW = 8
PLENS = (9, 14, 5, 14)          # prompt lengths: ragged left padding, two rows without any
A1 = (1, 4, 7, 12)              # forced members (+ EOS): rows end at steps 2, 5, 8 = MAX_NEW; 12 > MAX_NEW: the row never ends
Q2 = (3, 6, 1, 4)
A2 = (2, 1, 5, 3)               # every row ends: the loop stops early and the rows' run-ahead slots stay outside every window
Q3 = (2, 0, 3, 1)               # an empty follow-up row: legal behind a pending id
A3 = (1, 2, 1, 2)


def rows(cfg, lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(3, cfg.dec_vocab, int(n)) for n in lens]


def forced(members):
    return TokenTrie.per_row([TokenTrie([[int(t) for t in m]], end_token_id=EOS) for m in members])


def gen_kw(members, pad=PAD, max_new=MAX_NEW, **kw):
    base = dict(pad_token_id=pad, eos_token_id=[EOS], max_new_tokens=max_new, return_dict_in_generate=True, output_logits=True,
                output_token_logprobs=True, prefix_allowed_tokens_fn=forced(members))
    base.update(kw)
    return base


def answers(out):
    """ids[b, : n_b] of every row as int arrays (its EOS included)"""
    seq = out.sequences.cpu()
    n = counted_tokens(seq, [EOS]).tolist()
    return [seq[b, : n[b]].numpy() for b in range(seq.shape[0])]


def worst_rel_l2(got, ref) -> float:
    """max over (row, step) of the rel-L2 of a row's logits; no pair left out"""
    assert len(got) == len(ref) and len(got) > 0, (len(got), len(ref))
    worst = 0.0
    for g, p in zip(got, ref):
        g, p = g.double().cpu(), p.double().cpu()
        worst = max(worst, float(((g - p).norm(dim=1) / p.norm(dim=1).clamp_min(1e-30)).max()))
    return worst


def bitwise(a, b) -> bool:
    return len(a) == len(b) and all(pg.same(x, y) for x, y in zip(a, b))


def all_zero(x: torch.Tensor) -> bool:
    return x.numel() == 0 or not bool(x.contiguous().view(torch.int16).any())


# ------------------------------------------------------------------------------------------------ the export kernel, bit for bit
def export_vs_rectangle(model, sequences, T0: int) -> dict:
    """opus_llama_prefix_export_rows on the state a generate() call left against the rectangular opus_llama_prefix_export of the
    same cache re-indexed in torch."""
    cfg = model.cfg
    n_b = counted_tokens(sequences.cpu(), [EOS]).numpy()
    keep = n_b - 1
    R = len(keep)
    epoch = model.stat("cache_epoch")
    rk, rv, rkst = model.export_cache(epoch, R, T0 + int(keep.max()))
    kst = rkst.cpu().numpy()
    lengths, Tp, nks = plan_export_rows(kst, T0, keep)
    k, v, okst = model.export_cache_rows(keep, Tp)
    k2, v2, okst2 = model.export_cache_rows(keep, Tp)
    win = pad = True
    for r in range(R):
        a, e = int(kst[r]), T0 + int(keep[r])
        win &= pg.same(k[:, r, :, nks[r]:], rk[:, r, :, a:e]) and pg.same(v[:, r, :, nks[r]:], rv[:, r, :, a:e])
        pad &= all_zero(k[:, r, :, : nks[r]]) and all_zero(v[:, r, :, : nks[r]])
    wide_k, _, wide_kst = model.export_cache_rows(keep, Tp + 3)            # a wider snapshot: three more zero slots in front
    wide = all(pg.same(wide_k[:, r, :, nks[r] + 3:], k[:, r, :, nks[r]:]) and all_zero(wide_k[:, r, :, : nks[r] + 3]) for r in range(R))
    return dict(windows=bool(win), pads_zero=bool(pad), kstart=okst.cpu().numpy().tolist() == nks.tolist(),
                lengths_sum=bool((nks + lengths == Tp).all()), twice=pg.same(k, k2) and pg.same(v, v2) and torch.equal(okst, okst2),
                wider=bool(wide) and wide_kst.cpu().numpy().tolist() == (nks + 3).tolist(), nonzero=float(k.float().abs().max()) > 0,
                Tp=int(Tp), T0=int(T0), keep=keep.tolist(), kstart_live=kst.tolist(), crosses_64=bool(((kst < 64) & (T0 + keep > 64)).any()))


def turn1(model, seed, plens=PLENS, pad=PAD, **kw):
    cfg = model.cfg
    prompts, a1 = rows(cfg, plens, seed), rows(cfg, A1, seed + 3)
    ids, mask = pg.left_pad(prompts)
    out = model.generate(ids, attention_mask=mask, return_prefix=True, **gen_kw(a1, pad, **kw))
    return prompts, out, int(ids.shape[1])


def export_checks(model, seed, plens=PLENS) -> dict:
    """Item 1: behind a plain producer and behind a generate(prefix=...) producer; the handle generate() returned holds the same
    bits; the context is unchanged (the same decode step with and without the exports in front gives the same logits); bad
    arguments are refused and the context still works."""
    cfg = model.cfg
    obs = {}
    turn1(model, seed, plens)                                              # (warm: both runs below replay the same decode graph)
    prompts, out, T0 = turn1(model, seed, plens)
    tok =torch.full((len(plens),), 5, dtype=torch.long, device=model.device)
    lg_plain = model.decode_logits(tok).clone()                            # no export of ours in front of this step
    prompts, out, T0 = turn1(model, seed, plens)                           # the same call again
    o = export_vs_rectangle(model, out.sequences, T0)
    h = out.prefix
    keep = np.asarray(o["keep"])
    k, v, kst = model.export_cache_rows(keep, o["Tp"])
    o["handle_same_bits"] = pg.same(h._k, k) and pg.same(h._v, v) and torch.equal(h._kstart, kst) and h.slots == o["Tp"]
    seq = out.sequences.cpu()
    o["pending"] = h.pending.tolist() == [int(seq[b, keep[b]]) for b in range(len(keep))]
    o["lengths"] = h.lengths.tolist() == [T0 - a + int(kp) for a, kp in zip(o["kstart_live"], keep)]
    # refusals: a keep above the decode steps that ran, a negative one, a snapshot too narrow, too wide, another row count
    steps = int(seq.shape[1]) + 2                                          # (the loop runs at most 2 steps ahead)
    codes = []
    for bad_keep, bad_T in ((keep + steps, o["Tp"] + steps), (keep - 1 - keep.min(), o["Tp"]), (keep, o["Tp"] - 1),
                            (keep, cfg.max_prompt + cfg.max_new_tokens + 1), (keep[:-1], o["Tp"])):
        try:
            model.export_cache_rows(bad_keep, bad_T)
            codes.append(0)
        except _cabi.OpusError as e:
            codes.append(e.code)
    o["refusal_codes"] = codes
    k3, v3, _ = model.export_cache_rows(keep, o["Tp"])
    o["works_after_refusals"] = pg.same(k3, k) and pg.same(v3, v)
    o["context_unchanged"] = pg.same(model.decode_logits(tok), lg_plain)
    obs["plain"] = o
    # behind a generate(prefix=...) producer
    q2, a2 = rows(cfg, Q2, seed + 1), rows(cfg, A2, seed + 4)
    ids, mask = pg.left_pad(q2)
    out2 = model.generate(ids, attention_mask=mask, prefix=h, return_prefix=True, **gen_kw(a2))
    o2 = export_vs_rectangle(model, out2.sequences, h.slots + 1 + max(Q2))
    k, v, kst = model.export_cache_rows(np.asarray(o2["keep"]), o2["Tp"])
    o2["handle_same_bits"] = pg.same(out2.prefix._k, k) and pg.same(out2.prefix._v, v) and torch.equal(out2.prefix._kstart, kst)
    obs["behind"] = o2
    return obs


# ------------------------------------------------------------------------------------------------ turn 2 = the concatenated conversation
def chain(model, seed, n_turns=3, pad=PAD, plens=PLENS, max_new=MAX_NEW, **kw):
    """The conversation as a chain of generate calls: -> (outs, handles, inputs per turn, history rows before each turn)."""
    cfg = model.cfg
    qs = [rows(cfg, plens, seed), rows(cfg, Q2, seed + 1), rows(cfg, Q3, seed + 2)]
    ans = [rows(cfg, A1, seed + 3), rows(cfg, A2, seed + 4), rows(cfg, A3, seed + 5)]
    outs, handles, cats = [], [], []
    hist = [np.zeros(0, dtype=np.int64) for _ in plens]
    for t in range(n_turns):
        ids, mask = pg.left_pad(qs[t])
        hist = [np.concatenate([h, q]).astype(np.int64) for h, q in zip(hist, qs[t])]
        cats.append(hist)
        extra = dict(prefix=handles[-1]) if t else {}
        out = model.generate(ids, attention_mask=mask, return_prefix=True, **extra, **gen_kw(ans[t], pad, max_new, **kw))
        outs.append(out)
        handles.append(out.prefix)
        hist = [np.concatenate([h, a]).astype(np.int64) for h, a in zip(hist, answers(out))]
    return outs, handles, qs, ans, cats


def plain_turn(model, cat, members, pad=PAD, max_new=MAX_NEW):
    cids, cmask = pg.left_pad(cat)
    return model.generate(cids, attention_mask=cmask, **gen_kw(members, pad, max_new)), cids, cmask


def turns_vs_concat(model, seed, n_turns=3, scoring=True, new_context=True) -> dict:
    """Item 2: every later turn through the handle against plain generate() on the left-padded concatenation, same forcing."""
    outs, handles, qs, ans, cats = chain(model, seed, n_turns)
    h1 = handles[0]
    keep1 = (h1._k.clone(), h1._v.clone(), h1._kstart.clone(), h1.pending.clone())
    obs = {"ids_forced": all(np.array_equal(a[: len(m)], m[: len(a)]) for a, m in zip(answers(outs[0]), ans[0]))}
    for t in range(1, n_turns):
        plain, cids, cmask = plain_turn(model, cats[t], ans[t])
        o = dict(ids_equal=bool(torch.equal(plain.sequences, outs[t].sequences)), rel_l2=worst_rel_l2(outs[t].logits, plain.logits),
                 steps=len(plain.logits))
        if scoring:
            whole = model.cache_prefix(cids, attention_mask=cmask)
            got = answers(outs[t])
            sc = model.score_continuations(whole, [torch.from_numpy(a) for a in got])
            lp = outs[t].token_logprobs.cpu()
            o["teacher_forced_abs"] = max(float((lp[b, : len(a)] - sc.token_logprobs[b, : len(a)].cpu()).abs().max())
                                          for b, a in enumerate(got))
        obs[f"turn{t + 1}"] = o
    if new_context:
        other = model.new_context()
        ids, mask = pg.left_pad(qs[1])
        again = other.generate(ids, attention_mask=mask, prefix=h1, **gen_kw(ans[1]))
        obs["new_context_bitwise"] = bool(torch.equal(again.sequences, outs[1].sequences)) and bitwise(again.logits, outs[1].logits)
    obs["handle_unchanged"] = all(pg.same(a, b) if a.dtype != torch.int64 else bool(torch.equal(a, b))
                                  for a, b in zip(keep1, (h1._k, h1._v, h1._kstart, h1.pending)))
    return obs


# ------------------------------------------------------------------------------------------------ seal and rank, extend
def seal_and_rank(model, seed) -> dict:
    """Item 3: a sealed pending handle ranks continuations as the prefilled conversation does; a handle extended by teacher-forced
    ids generates as the unextended one with those ids in front of the suffix."""
    cfg = model.cfg
    prompts, out, _ = turn1(model, seed)
    h = out.prefix
    R = len(prompts)
    sealed = model.cache_prefix(torch.zeros((R, 0), dtype=torch.long), prefix=h)
    conts = [torch.from_numpy(c) for c in rows(cfg, (3, 2, 4, 1), seed + 9)]
    got = model.score_continuations(sealed, conts)
    live_ok = (not sealed.detached) and sealed.pending is None and sealed.slots == h.slots + 1 and \
        sealed.lengths.tolist() == (h.lengths + 1).tolist()
    cat = [np.concatenate([p, a]) for p, a in zip(prompts, answers(out))]
    cids, cmask = pg.left_pad(cat)
    ref = model.score_continuations(model.cache_prefix(cids, attention_mask=cmask), conts)
    obs = dict(sealed_is_live=bool(live_ok), rank_abs=float((got.token_logprobs.cpu() - ref.token_logprobs.cpu()).abs().max()),
               n_tokens=got.n_tokens.tolist())
    ext_rows, suf, a2 = rows(cfg, (2, 3, 1, 2), seed + 10), rows(cfg, Q2, seed + 1), rows(cfg, A2, seed + 4)
    eids, emask = pg.left_pad(ext_rows)
    ext = model.cache_prefix(eids, attention_mask=emask, prefix=h)
    obs["extended_lengths"] = ext.lengths.tolist() == [int(l) + 1 + len(e) for l, e in zip(h.lengths.tolist(), ext_rows)]
    sids, smask = pg.left_pad(suf)
    a = model.generate(sids, attention_mask=smask, prefix=ext, **gen_kw(a2))
    jids, jmask = pg.left_pad([np.concatenate([e, s]) for e, s in zip(ext_rows, suf)])
    b = model.generate(jids, attention_mask=jmask, prefix=h, **gen_kw(a2))
    obs["extend_ids_equal"] = bool(torch.equal(a.sequences, b.sequences))
    obs["extend_rel_l2"] = worst_rel_l2(a.logits, b.logits)
    return obs


# ------------------------------------------------------------------------------------------------ ChatSession
def session(model, seed) -> dict:
    """Item 4: three turns through ChatSession equal the chain of generate calls; rewind(1) + ask repeats the turn bit for bit;
    sampling with a fixed seed runs and repeats itself.  pad_token_id == eos_token_id, as the reference's drivers pass it."""
    import opus_pllm_amd as opa
    outs, handles, qs, ans, _ = chain(model, seed, 3, pad=EOS)
    chat = opa.ChatSession(model)
    got = []
    for t in range(3):
        ids, mask = pg.left_pad(qs[t])
        got.append(chat.ask(ids, attention_mask=mask, **{k: v for k, v in gen_kw(ans[t], EOS).items() if k != "return_dict_in_generate"}))
    obs = dict(ids_equal=all(bool(torch.equal(g.sequences, o.sequences)) for g, o in zip(got, outs)),
               logits_bitwise=all(bitwise(g.logits, o.logits) for g, o in zip(got, outs)),
               turns=len(chat.turns), lengths=chat.lengths.tolist() == handles[2].lengths.tolist(),
               handle_bytes=chat.prefix.nbytes())
    chat.rewind(1)
    ids, mask = pg.left_pad(qs[2])
    again = chat.ask(ids, attention_mask=mask, **gen_kw(ans[2], EOS))
    obs["rewind_bitwise"] = bool(torch.equal(again.sequences, got[2].sequences)) and bitwise(again.logits, got[2].logits) and \
        len(chat.turns) == 3
    try:
        chat.rewind(2)
        obs["rewind_past_kept"] = "allowed"
    except ValueError:
        obs["rewind_past_kept"] = "refused"
    samp = []
    for _ in range(2):
        c = opa.ChatSession(model, keep_handles=True)
        seqs = []
        for t in range(3):
            ids, mask = pg.left_pad(qs[t])
            o = c.ask(ids, attention_mask=mask, pad_token_id=EOS, eos_token_id=[EOS], max_new_tokens=6, do_sample=True, seed=5 + t,
                      temperature=1.0, top_p=0.9)
            seqs.append(o.sequences.cpu())
        c.rewind(2)                                                         # every handle kept: two steps back are allowed
        samp.append(seqs)
    obs["sampling_repeats"] = all(bool(torch.equal(a, b)) for a, b in zip(*samp))
    obs["sampling_turns"] = len(samp[0])
    return obs


# ------------------------------------------------------------------------------------------------ Llama-3-8B widths
def widths(model, seed) -> dict:
    """Item 5: turn 2 behind the exported handle against plain generate() on the concatenation, beside the quantity the parent
    already bounds on the same rows: generate(prefix=cache_prefix(prompt + a1[:-1])) - a PREFILLED history - against plain."""
    outs, handles, qs, ans, cats = chain(model, seed, 2)
    plain, _, _ = plain_turn(model, cats[1], ans[1])
    a1 = answers(outs[0])
    hist = [np.concatenate([p, a[:-1]]) for p, a in zip(qs[0], a1)]
    hids, hmask = pg.left_pad(hist)
    pre = model.cache_prefix(hids, attention_mask=hmask, detach=True)
    sids, smask = pg.left_pad([np.concatenate([a[-1:], q]) for a, q in zip(a1, qs[1])])
    behind = model.generate(sids, attention_mask=smask, prefix=pre, **gen_kw(ans[1]))
    return dict(ids_equal=bool(torch.equal(plain.sequences, outs[1].sequences)) and bool(torch.equal(plain.sequences, behind.sequences)),
                decoded_history_rel_l2=worst_rel_l2(outs[1].logits, plain.logits),
                prefilled_history_rel_l2=worst_rel_l2(behind.logits, plain.logits), steps=len(plain.logits))
