"""Checks of prompt-lookup decoding shared by tests/test_gpu_lookup.py (fp16 build) and tests/bf16_lookup_check.py (the bf16
build, a child process): each returns observations; the callers hold the bounds.  The twin is tests/lookup_ref.py."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, synth
import lookup_ref as LR


def make_model(cfg, dev, seed=0, **kw):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    return OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, seed, dev, **kw), dev)


def wide_cfg(max_batch=64):
    """Llama-3-8B widths, 2 layers (tests/test_gpu_w8.py's wide pair, with room for prompts of 64 + 16 positions)."""
    return opa.OpusConfig(enc_layers=1, enc_dim=64, enc_heads=4, enc_ffn=128, proj_dim=64, switch_depth=1, n_prot_tokens=1,
                          dec_layers=2, dec_dim=4096, dec_heads=32, dec_kv_heads=8, dec_head_dim=128, dec_ffn=14336,
                          dec_vocab=32768, dec_rope_theta=500000.0, max_batch=max_batch, max_enc_tokens=34, max_prompt=96,
                          max_new_tokens=24).validate()


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ the draft kernel
def draft_histories(R: int, L: int, vocab: int, seed: int):
    """R histories of length L over a small vocabulary (matches abound), with sentinels sprinkled into some rows."""
    rng = random.Random(seed)
    rows = []
    for r in range(R):
        h = [rng.randrange(vocab) for _ in range(L)]
        if r % 3 == 1 and L > 4:
            for _ in range(max(1, L // 40)):
                h[rng.randrange(L)] = -1
        rows.append(h)
    return rows


def sentinel_histories():
    return [[5, 6, -1, 7, 5, 6],               # the only earlier "5 6" is followed by the sentinel: falls back to m = 1 ("6" -> none valid)
            [1, 2, 3, 9, -1, 1, 2],            # draft 3 9, cut in front of the sentinel
            [4, -1, 8, 4, -1],                 # the tail holds the sentinel at every m: no draft
            [7, 8, 9, -1, 3, 7, 8],            # prompt | corpus separator: the match is in the prompt, the draft stops at the separator
            [3, 3, 3, 3],                      # overlapping windows: first start wins
            [2]]                               # a single id: nothing to match


def run_draft(lib, ctx, dev, rows, k, m):
    R, L = len(rows), max(1, max(len(h) for h in rows))
    hist = np.full((R, L), -1, dtype=np.int32)
    for r, h in enumerate(rows):
        hist[r, :len(h)] = h
    d_hist = torch.from_numpy(hist).to(dev)
    d_len = torch.tensor([len(h) for h in rows], dtype=torch.int32, device=dev)
    d_draft = torch.full((R, k), -7, dtype=torch.int32, device=dev)
    d_dl = torch.full((R,), -7, dtype=torch.int32, device=dev)
    _cabi.check(lib.opus_debug_lookup_draft(ctx, d_hist.data_ptr(), L, d_len.data_ptr(), R, k, m, d_draft.data_ptr(), d_dl.data_ptr(), None))
    torch.cuda.synchronize()
    return d_draft.cpu().tolist(), d_dl.cpu().tolist()


def draft_mismatches(lib, ctx, dev, rows, k, m):
    got, got_len = run_draft(lib, ctx, dev, rows, k, m)
    bad = []
    for r, h in enumerate(rows):
        want = LR.draft(h, k, m)
        if got_len[r] != len(want) or got[r][:len(want)] != want or any(t != 0 for t in got[r][len(want):]):
            bad.append((r, len(h), want, got[r], got_len[r]))
    return bad


# ------------------------------------------------------------------------------------------------ the commit kernel
def run_accept(lib, ctx, dev, st: LR.State, x, y, draft_len, pre, eos=(), stop=()):
    """lookup_accept_kernel on a copy of the twin's state; returns (ids, fin, step, next, n_unf, words)."""
    R, n = len(y), len(y[0])
    t = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)                       # noqa: E731
    d_y, d_x, d_dl = t(y), t([row[:n] for row in x]), t(list(draft_len))
    d_ids, d_fin, d_step, d_next, d_nunf = t(st.ids), t(st.fin), t([st.step]), t(st.next), t(st.n_unf)
    words = (C.c_int32 * 4)()
    e = (C.c_int32 * max(1, len(eos)))(*eos)
    s_ = (C.c_int32 * max(1, len(stop)))(*stop)
    _cabi.check(lib.opus_debug_lookup_accept(ctx, d_y.data_ptr(), d_x.data_ptr(), d_dl.data_ptr(), R, n, pre, d_ids.data_ptr(), st.stride,
                                             d_fin.data_ptr(), d_step.data_ptr(), e, len(eos), st.pad, s_, len(stop), d_next.data_ptr(),
                                             d_nunf.data_ptr(), words, None))
    return d_ids.cpu().tolist(), d_fin.cpu().tolist(), int(d_step.item()), d_next.cpu().tolist(), d_nunf.cpu().tolist(), list(words)


def commit_cases(gold_ids):
    """Drafts crafted from golden ids (3 rows x 12): (name, state set-up, x, y, draft_len, eos, stop).  y are the model's ids (the
    golden row from the current column on), x the fed tokens."""
    G = [list(map(int, r)) for r in gold_ids]
    R, stride, pad = 3, 12, 2

    def state(step, fin=(0, 0, 0)):
        st = LR.State(R, stride, pad)
        st.step = step
        st.fin = list(fin)
        for b in range(R):
            for c in range(step + 1):
                st.ids[b][c] = pad if fin[b] else G[b][c]
                st.n_unf[c] = sum(1 for f in fin if not f)
            st.next[b] = st.ids[b][step]
        return st

    def xy(step, n, wrong_from):       # row b's draft is right up to wrong_from[b] ids, then wrong
        x, y = [], []
        for b in range(R):
            yb = (G[b] + [40 + b] * n)[step + 1: step + 1 + n]          # (ids past the matrix: what the model would say next)
            xb = [G[b][step]] + [yb[j] if j < wrong_from[b] else (yb[j] + 1) % 90 + 3 for j in range(n - 1)]
            x.append(xb)
            y.append(yb)
        return x, y
    cases = []
    x, y = xy(2, 5, (0, 0, 0)); cases.append(("accept_none", state(2), x, y, [4, 4, 4], (), ()))
    x, y = xy(2, 5, (4, 4, 4)); cases.append(("accept_all", state(2), x, y, [4, 4, 4], (), ()))
    x, y = xy(2, 5, (2, 2, 2)); cases.append(("partial", state(2), x, y, [4, 4, 4], (), ()))
    x, y = xy(2, 5, (4, 1, 3)); cases.append(("rows_differ_min_rules", state(2), x, y, [4, 4, 4], (), ()))
    x, y = xy(2, 5, (4, 4, 4)); cases.append(("short_draft_len_rules", state(2), x, y, [4, 2, 3], (), ()))
    x, y = xy(1, 6, (5, 5, 5)); cases.append(("eos_accepted", state(1), x, y, [5, 5, 5], (G[1][4],), ()))
    x, y = xy(1, 6, (1, 1, 1)); cases.append(("eos_rejected", state(1), x, y, [5, 5, 5], (G[1][4],), ()))
    x, y = xy(8, 6, (5, 5, 5)); cases.append(("budget_inside_chain", state(8), x, y, [5, 5, 5], (), ()))
    x, y = xy(3, 5, (4, 0, 4)); cases.append(("finished_row_ignored", state(3, (0, 1, 0)), x, y, [4, 4, 4], (), ()))
    x, y = xy(2, 5, (4, 4, 4)); cases.append(("stop_sequence", state(2), x, y, [4, 4, 4], (), (G[0][4], G[0][5])))
    return cases


# ------------------------------------------------------------------------------------------------ verify_step against prefill
def random_prompt(cfg, R, Tp, pads, seed):
    """ids [R, Tp] left-padded by pads[r] (the pad id 2), tokens from [3, V)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, cfg.dec_vocab, (R, Tp), generator=g)
    mask = torch.ones((R, Tp), dtype=torch.bool)
    for r in range(R):
        ids[r, :pads[r]] = 2
        mask[r, :pads[r]] = False
    return ids, mask


def embed(model, ids):
    return model.get_model().embed_tokens(ids).to(_cabi.operand_dtype())


def verify_vs_prefill(model, R, Tp, pads, n, seed=0):
    """One verify pass of n positions behind a prompt of Tp slots against prefill_logits of the prompt extended by 1 .. n of the
    pass's tokens: the worst rel-L2 over the n positions (every position is compared)."""
    cfg = model.cfg
    ids, mask = random_prompt(cfg, R, Tp, pads, seed)
    g = torch.Generator().manual_seed(seed + 1)
    toks = torch.randint(3, cfg.dec_vocab, (R, n), generator=g)
    ref = []
    for j in range(n):
        full = torch.cat([ids, toks[:, :j + 1]], 1)
        fm = torch.cat([mask, torch.ones((R, j + 1), dtype=torch.bool)], 1)
        ref.append(model.prefill_logits(embed(model, full), fm).cpu())
    model.prefill_logits(embed(model, ids), mask)
    logits, arg, a = model.verify_step(toks)
    return {"rel_l2": max(rel_l2(logits[:, j], ref[j]) for j in range(n)), "a": a,
            "argmax_equal": bool(torch.equal(arg.cpu().long(), logits.cpu().argmax(-1)))}


def export_kv(model, R, T):
    """K, V [layers, R, kv heads, T, hd] of the live cache behind prefill_with_epoch (opus_llama_prefix_export checks its epoch)."""
    cfg = model.cfg
    k = torch.empty((cfg.dec_layers, R, cfg.dec_kv_heads, T, cfg.dec_head_dim), dtype=_cabi.operand_dtype(), device=model.device)
    v = torch.empty_like(k)
    s = model._enter()
    try:
        _cabi.check(model._lib.opus_llama_prefix_export(model._ctx, model_epoch(model), R, T, k.data_ptr(), v.data_ptr(), None, s))
    finally:
        model._leave()
    torch.cuda.synchronize()
    return k.cpu(), v.cpu()


def model_epoch(model):
    return int(getattr(model, "_lookup_test_epoch"))


def prefill_with_epoch(model, emb, mask):
    """prefill through opus_llama_prefix (the same prefill, plus the epoch handle the export checks)."""
    B, T, _ = emb.shape
    emb = emb.to(model.device, _cabi.operand_dtype()).contiguous()
    mask = mask.to(model.device).to(torch.uint8).contiguous()
    s = model._enter()
    with torch.cuda.stream(model._stream):
        logits = torch.empty((B, model.cfg.dec_vocab), dtype=torch.float32, device=model.device)
        rows = torch.empty((B, model.cfg.dec_dim), dtype=torch.float32, device=model.device)
        ep = C.c_int64(0)
        _cabi.check(model._lib.opus_llama_prefix(model._ctx, emb.data_ptr(), mask.data_ptr(), B, T, logits.data_ptr(), rows.data_ptr(),
                                                 C.byref(ep), s))
    model._leave()
    model._lookup_test_epoch = ep.value
    return logits


def verify_kv(model, R, Tp, pads, n, seed=0):
    """The K / V a verify pass appends at slots Tp .. Tp + n - 1.
    (1) The decode attention's rule (tests/attn_decode_checks.py), on the last layer, whose projections the context still holds:
        the appended key against the pass's own rotated k, the appended value against its own v - both bit for bit (the rotation
        runs in front of the append here, so the key is exact too).
    (2) Every layer against the prefill of the extended prompt, which reaches the same numbers through other GEMM kernels:
        max |diff| / max |ref| of keys and values, and whether the values happen to be bit-equal.
    (3) The prompt's slots are what they were before the pass, bit for bit."""
    cfg = model.cfg
    nh, nkv, hd = cfg.dec_heads, cfg.dec_kv_heads, cfg.dec_head_dim
    ids, mask = random_prompt(cfg, R, Tp, pads, seed)
    g = torch.Generator().manual_seed(seed + 1)
    toks = torch.randint(3, cfg.dec_vocab, (R, n), generator=g)
    full = torch.cat([ids, toks], 1)
    fm = torch.cat([mask, torch.ones((R, n), dtype=torch.bool)], 1)
    prefill_with_epoch(model, embed(model, full), fm)
    rk, rv = export_kv(model, R, Tp + n)
    prefill_with_epoch(model, embed(model, ids), mask)
    k0, v0 = export_kv(model, R, Tp)
    model.verify_step(toks, return_logits=False)
    qkv = torch.empty((R * n, (nh + 2 * nkv) * hd), dtype=_cabi.operand_dtype(), device=model.device)
    _cabi.check(model._lib.opus_debug_last_qkv(model._ctx, qkv.data_ptr(), R * n, None))
    k, v = export_kv(model, R, Tp + n)
    qkv = qkv.cpu().view(R, n, nh + 2 * nkv, hd)
    own_k = qkv[:, :, nh:nh + nkv].permute(0, 2, 1, 3)             # [R, kv, n, hd]
    own_v = qkv[:, :, nh + nkv:].permute(0, 2, 1, 3)
    bits = lambda t: t.contiguous().view(torch.int16)               # noqa: E731
    vis = torch.zeros((R, Tp), dtype=torch.bool)
    for r in range(R):
        vis[r, pads[r]:] = True                                    # (slots under the left padding hold nothing defined)
    old = vis[None, :, None, :, None].expand_as(k0)
    nk, nv, rnk, rnv = k[..., Tp:, :].double(), v[..., Tp:, :].double(), rk[..., Tp:, :].double(), rv[..., Tp:, :].double()
    return {"last_layer_key_exact": bool(torch.equal(bits(k[-1][..., Tp:, :]), bits(own_k))),
            "last_layer_value_exact": bool(torch.equal(bits(v[-1][..., Tp:, :]), bits(own_v))),
            "key_err": float((nk - rnk).abs().max() / rnk.abs().max()),
            "value_err": float((nv - rnv).abs().max() / rnv.abs().max()),
            "value_bit_equal_to_prefill": bool(torch.equal(bits(v[..., Tp:, :]), bits(rv[..., Tp:, :]))),
            "prompt_slots_untouched": bool(torch.equal(bits(k[..., :Tp, :][old]), bits(k0[old])) and
                                           torch.equal(bits(v[..., :Tp, :][old]), bits(v0[old])))}


def stale_slots(model, R=3, Tp=30, seed=3):
    """Slots beyond Tp + a keep the K / V of rejected positions; nothing may read them.
    State A:  a pass of n = 8 whose draft is wrong from position 2 on (a = 1), then a pass of n = 4 and a plain decode step.
    State A': the same, with OTHER wrong ids at positions 2 .. 7: the accepted positions run in the same launches on the same
              inputs, so their K / V are A's bit for bit, and only the stale slots differ.  Second pass and plain step have to
              be bit-identical to A's: this is the property, exact by construction.
    State B:  a pass of n = 2 with the right draft (no stale slot at all), then the same pass of n = 4 and the plain step.  Its
              accepted positions went through launches of another shape (6 rows instead of 24: other GEMM row tiles, another
              stacking of the attention's queries), so their K / V differ from A's in the last bits for a reason that has
              nothing to do with stale slots; the rel-L2 distance of A's and B's logits is returned, to be held to the bound of
              two launch shapes of one computation ("decode step against prefill of the longer prompt")."""
    cfg = model.cfg
    ids, mask = random_prompt(cfg, R, Tp, [0, 7, 3][:R], seed)
    emb = embed(model, ids)
    x0 = model.prefill_logits(emb, mask).argmax(-1).cpu()
    y0 = model.verify_step(x0[:, None])[1][:, 0].cpu().long()                     # (the pass's own kernels decide y_0)
    outs, nxts = {}, {}
    for state in ("A", "A'", "B"):
        model.prefill_logits(emb, mask)
        if state == "B":
            toks = torch.cat([x0[:, None], y0[:, None]], 1)
        else:
            wrong = torch.randint(3, cfg.dec_vocab, (R, 6), generator=torch.Generator().manual_seed(seed + (5 if state == "A" else 6)))
            toks = torch.cat([x0[:, None], y0[:, None], wrong], 1)
        lg, arg, a = model.verify_step(toks)
        if state != "B":
            # the draft is wrong at position 2 for every row (a random id equals the arg-max with probability 1 / V)
            assert bool((arg[:, 1].cpu().long() != toks[:, 2]).all())
        assert a == 1, (state, a)
        nxts[state] = arg[:, 1].cpu().long()                                      # y_1: the last committed id
        second = torch.cat([nxts[state][:, None],
                            torch.randint(3, cfg.dec_vocab, (R, 3), generator=torch.Generator().manual_seed(seed + 9))], 1)
        lg2, arg2, a2 = model.verify_step(second, draft_len=torch.zeros(R, dtype=torch.int32))   # (a = 0: one position kept)
        lg3 = model.decode_logits(arg2[:, 0].long())
        outs[state] = (lg2.cpu(), lg3.cpu(), a2)
    assert torch.equal(nxts["A"], nxts["A'"]) and torch.equal(nxts["A"], nxts["B"])
    return {"second_pass_identical": bool(torch.equal(outs["A"][0], outs["A'"][0])),
            "plain_step_identical": bool(torch.equal(outs["A"][1], outs["A'"][1])),
            "a2": [outs["A"][2], outs["A'"][2], outs["B"][2]],
            "b_second_pass_identical": bool(torch.equal(outs["A"][0], outs["B"][0])),
            "b_plain_step_identical": bool(torch.equal(outs["A"][1], outs["B"][1])),
            "b_second_pass_rel_l2": rel_l2(outs["A"][0], outs["B"][0]), "b_plain_step_rel_l2": rel_l2(outs["A"][1], outs["B"][1])}


# ------------------------------------------------------------------------------------------------ end to end
def ragged_inputs(cfg, B=3):
    lens = [(14, 5), (9, 2), (11, 3), (7, 1)]
    rows = [synth.synth_prompt_ids(cfg.dec_vocab, i, n_text=lens[i % 4][0], seq_pos=lens[i % 4][1]) for i in range(B)]
    width = max(len(r) for r in rows)
    ids = torch.full((B, width), 2, dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, width - len(r):] = torch.tensor(r)
    return ids, ids != 2, [synth.synth_protein(20 + 7 * i, i) for i in range(B)]


def e2e(model, ids, mask, seqs, max_new, k=7, **kw):
    """(plain ids, lookup ids, stats) of the same greedy call."""
    base = dict(attention_mask=mask, pad_token_id=2, do_sample=False, max_new_tokens=max_new)
    base.update(kw)
    lookup_ids = base.pop("lookup_ids", None)
    plain = model.generate(ids, seqs, **base).cpu()
    out = model.generate(ids, seqs, prompt_lookup_num_tokens=k, return_dict_in_generate=True,
                         **({} if lookup_ids is None else {"lookup_ids": lookup_ids}), **base)
    return plain, out.sequences.cpu(), out.stats
