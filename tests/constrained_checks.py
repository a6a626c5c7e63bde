"""Checks of constrained decoding (generate(prefix_allowed_tokens_fn=TokenTrie)) shared by tests/test_gpu_constrained.py
(fp16-operand build) and its bf16 child process (tests/bf16_constrained_check.py).  Each returns a dict of observations; the
callers assert the bounds.  Test infrastructure, not product code."""
from __future__ import annotations

import json
import os
import threading

import numpy as np
import torch

from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TokenTrie
import constrained_ref as cref
import gen_scores_checks as gsc
import logits_proc_checks as lpc
import logits_proc_ref as lpr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, bad_words_ids=lpc.BAD, min_new_tokens=4)


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.detach().float().cpu().contiguous().view(torch.int32)


def big_members(n: int = 50000, seed: int = 0, lo: int = 4, hi: int = 16, first: int = 6000, rest: int = 64, base: int = 1000):
    """n members of lo to hi ids: the first id out of `first` ids (a root with thousands of children), the others out of `rest`
    ids, none twice within a member (no processor can then ban a member's only continuation), all ids >= base."""
    rng = np.random.default_rng(seed)
    out = []
    for ln in rng.integers(lo, hi + 1, size=n):
        tail = rng.permutation(rest)[: ln - 1] + base + first
        out.append([int(base + rng.integers(0, first))] + [int(t) for t in tail])
    return out


# ------------------------------------------------------------------------------------------------ kernel level
def _history(rng, tab, row, L, kind, V):
    """L ids for `row`: 'on' follows allowed ids (an end id only when nothing else is allowed), 'leave' takes an id that is
    not allowed half way, 'end' emits an end id as soon as a member completes and pads after it."""
    s, h = int(tab.start[row if len(tab.start) > 1 else 0]), []
    end = int(tab.end_ids[0])
    for i in range(L):
        ids = tab.edge_tok[tab.edge_off[s]: tab.edge_off[s + 1]]
        if kind == "leave" and i == L // 2:
            t = int(rng.integers(0, V))
        elif len(ids) == 0 or (kind == "end" and tab.completing[s]):
            t = end
        else:
            t = int(ids[int(rng.integers(0, len(ids)))])
        h.append(t)
        s = tab.step(s, t)
    return h


_BIG = {}


def _tables(V: int, B: int, big: bool, vocab: int):
    """Tries whose ids lie under V and under the context's vocabulary (opus_set_token_constraint checks them against it)."""
    rng = np.random.default_rng(V + B)
    top = min(V, vocab)
    end = [top - 1, top - 7]
    small = lambda n, hi=6: [[int(t) for t in rng.integers(0, min(V, 4000) - 8, size=int(rng.integers(1, hi + 1)))]    # noqa: E731
                            for _ in range(n)]
    sepid = min(V, 4000) - 5                                            # (outside the members' ids)
    out = {"one": TokenTrie(small(1), end_token_id=end), "m24": TokenTrie(small(24), end_token_id=end),
           "sep": TokenTrie(small(24), end_token_id=end, separator=[sepid]),
           "sep3": TokenTrie(small(40, 16), end_token_id=end, separator=[sepid, sepid - 1, sepid]),
           "rows": TokenTrie.per_row([TokenTrie(small(3 + b % 5), end_token_id=end, separator=[sepid] if b % 3 == 0 else None)
                                      for b in range(B)])}
    if big:                                                             # (built once: the same ids for both large V)
        if top not in _BIG:
            _BIG[top] = (TokenTrie(big_members(lo=1), end_token_id=end),
                         TokenTrie(big_members(5000, seed=1, lo=1), end_token_id=end, separator=[top - 20, top - 21]))
        out["m50000"], out["m50000sep"] = _BIG[top]
    return out


def kernel(model, dev, lengths=(0, 1, 17, 255)):
    """opus_debug_token_constraint against the restatement: -inf exactly where the restatement has it, every other entry
    bit-identical to the input, the state words equal to the host walk of the compiled table."""
    lib = _cabi.lib()
    s = torch.cuda.current_stream(dev)
    g = torch.Generator().manual_seed(5)
    res = {}
    for V in (96, 128256, 152064):
        for B in (1, 64):
            x = torch.randn(B, V, generator=g) * 4
            for name, trie in _tables(V, B, V > 96, model.cfg.dec_vocab).items():
                tab = trie.compiled()
                model._set_token_constraint(trie)
                rng = np.random.default_rng(len(name) + V)
                for L in lengths:
                    for kind in (("on",) if L == 0 else ("on", "leave", "end")):
                        if name.startswith("m50000") and (L, kind) not in ((0, "on"), (1, "on"), (17, "leave"), (255, "end"), (17, "on")):
                            continue
                        hist = [_history(rng, tab, b, L, kind, V) for b in range(B)]
                        stride = L + 3
                        hd = torch.zeros((B, stride), dtype=torch.int32)
                        if L:
                            hd[:, :L] = torch.tensor(hist, dtype=torch.int32)
                        d_x, d_h = x.to(dev), hd.to(dev)
                        d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
                        _cabi.check(lib.opus_debug_token_constraint(model._ctx, d_x.data_ptr(), B, V, d_h.data_ptr(), stride, L,
                                                                    d_st.data_ptr(), s.cuda_stream))
                        torch.cuda.synchronize(dev)
                        want = cref.process(x, hist, trie)
                        got = d_x.cpu()
                        banned = torch.isinf(want) & (want < 0)
                        states = [tab.walk(b, hist[b]) for b in range(B)]
                        res[f"V{V}_B{B}_{name}_L{L}_{kind}"] = {
                            "banned_equal": bool(torch.equal(torch.isinf(got) & (got < 0), banned)),
                            "allowed_identical": bool(torch.equal(_bits(got)[~banned], _bits(x)[~banned])),
                            "state_equal": d_st.cpu().tolist() == states,
                            "allowed": int((~banned).sum()), "in_end_state": int(sum(1 for v in states if v == 0)),
                            "widest": int((~banned).sum(1).max())}
    model._set_token_constraint(None)
    return res


# ------------------------------------------------------------------------------------------------ generate level
def _fixture():
    gp = dict(np.load(os.path.join(GOLD, "generate_constrained_micro.npz")))
    g = dict(np.load(os.path.join(GOLD, "generate_micro.npz")))
    seqs = json.load(open(os.path.join(GOLD, "generate_micro.seqs.json")))
    return gp, torch.from_numpy(g["ids"]), torch.from_numpy(g["mask"]), seqs


def fixture_fn(gp, tag):
    spec = json.loads(str(gp[tag + ".spec"]))
    tries = [TokenTrie(t["members"], end_token_id=int(gp["end"]), separator=t["sep"]) for t in spec["tries"]]
    return TokenTrie.per_row(tries) if spec["per_row"] else tries[0]


def golden(model):
    """The micro model against the reference's own constrained generate: EVERY id (the generator refused margins under 0.10)."""
    gp, ids, mask, seqs = _fixture()
    N, pad, end = int(gp["N"]), int(gp["pad"]), int(gp["end"])
    out = {}
    for tag in sorted({k.split(".")[0] for k in gp if "." in k}):
        kw = json.loads(str(gp[tag + ".kw"]))
        o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, do_sample=False, max_new_tokens=N, eos_token_id=[end],
                           return_dict_in_generate=True, output_scores=True, output_logits=True,
                           prefix_allowed_tokens_fn=fixture_fn(gp, tag), **kw)
        want = gp[tag + ".sequences"]
        got = o.sequences.cpu().numpy()
        rec = {"ids_equal": bool(got.shape == want.shape and np.array_equal(got, want)), "n": int(got.shape[1]),
               "N_ref": int(want.shape[1]), "got": got.tolist()}
        if rec["ids_equal"]:
            sc_w, lg_w = torch.from_numpy(gp[tag + ".scores"]), torch.from_numpy(gp[tag + ".logits"])
            sc, lg = torch.stack(o.scores).cpu(), torch.stack(o.logits).cpu()
            fin_o, fin_w = torch.isfinite(sc), torch.isfinite(sc_w)
            rec.update(inf_pattern_equal=bool(torch.equal(fin_o, fin_w)),
                       scores_rel_l2=lpc.gsc_rel_l2(torch.where(fin_w, sc, 0.0), torch.where(fin_w, sc_w, 0.0)),
                       logits_rel_l2=lpc.gsc_rel_l2(lg, lg_w))
        out[tag] = rec
    model._set_logits_processors(None)
    model._set_token_constraint(None)
    return out


def big(model, dev, B: int = 64, max_new: int = 16, sampling: bool = True, members=None):
    """Llama-3-8B shape under a 50 000-member trie, the constraint alone and with every other processor on: rows accepted by the
    host automaton, greedy ids = argmax(restatement(raw logits)), sampled scores = the warpers behind the restatement, every
    drawn id allowed, token_logprobs = fp64 log_softmax of the raw logits.  In the `_proc` modes the first ids the constrained
    greedy call chose for rows 0 to 7 are bad words as well (the root keeps thousands of other children), so those rows must
    take another member: the bans of the processors and of the constraint combine."""
    import oracle.sampling as osamp
    cfg = model.cfg
    ids, mask, seqs = gsc.batch(cfg, B)
    end = [cfg.dec_vocab - 3]
    members = members or big_members()
    trie = TokenTrie(members, end_token_id=end)
    tab = trie.compiled()
    plain = gsc._gen(model, ids, mask, seqs, max_new).cpu()
    res = {}
    modes = [("greedy", None, {}), ("greedy_proc", None, PROC)]
    if sampling:
        for s_ in gsc.SAMPLING:
            modes += [(f"T{s_['temperature']}_p{s_['top_p']}", s_, {}), (f"T{s_['temperature']}_p{s_['top_p']}_proc", s_, PROC)]
    first_ids = None
    for mode, samp, proc in modes:
        if proc:
            proc = dict(proc, bad_words_ids=list(proc["bad_words_ids"]) + [[t] for t in sorted(set(first_ids[:8]))])
        o = gsc._gen(model, ids, mask, seqs, max_new, samp, output_scores=True, output_logits=True, output_token_logprobs=True,
                     eos_token_id=end, prefix_allowed_tokens_fn=trie, **proc)
        seq = o.sequences.cpu()
        if first_ids is None:
            first_ids = seq[:, 0].tolist()               # (of the first mode: greedy under the constraint alone)
        n = seq.shape[1]
        cnt = o.n_tokens.cpu()
        rejected = sum(0 if _row_accepted(tab, b, seq[b].tolist(), end[0], pad=2) else 1 for b in range(B))
        mism = argmax_bad = near = drawn_bad = 0
        lp_worst, kept, total, widest = 0.0, 0, 0, 0
        for t in range(n):
            raw = o.logits[t].cpu()
            live = t < cnt
            pre = lpr.process(raw, seq[:, :t], eos=end, penalty=proc.get("repetition_penalty"),
                              ngram=proc.get("no_repeat_ngram_size", 0), bad=proc.get("bad_words_ids"),
                              min_new=proc.get("min_new_tokens", 0)) if proc else raw
            want = cref.process(pre, seq[:, :t], trie)
            tok = seq[:, t]
            widest = max(widest, int(torch.isfinite(want).sum(1).max()))
            lsm = torch.log_softmax(raw.double(), dim=-1)
            lp = o.token_logprobs[:, t].double().cpu()
            ref = lsm.gather(1, tok[:, None]).squeeze(1)
            if live.any():
                lp_worst = max(lp_worst, float((lp - ref)[live].abs().max()))
            allowed_tok = torch.isfinite(want.gather(1, tok[:, None])).squeeze(1)
            drawn_bad += int((~allowed_tok & live).sum())
            if samp is None:
                am = torch.from_numpy(np.argmax(want.numpy(), axis=1))
                argmax_bad += int((am != tok)[live].sum())
                mism += int((_bits(o.scores[t]) != _bits(want)).any(dim=1).sum())
            else:
                T = samp["temperature"]
                ours = o.scores[t].cpu()
                warped = osamp._warp(want / T, samp["top_p"], samp["top_k"])
                fo, fw = torch.isfinite(ours), torch.isfinite(warped)
                bad = (fo ^ fw) & live[:, None]
                total += int(fo[live].numel())
                kept += int(fo[live].sum())
                if bad.any():
                    p = torch.exp(want / T - (want / T).max(dim=1, keepdim=True).values).double()
                    thr = torch.where(fw, p, torch.full_like(p, 2.0)).min(dim=1, keepdim=True).values
                    close = (p - thr).abs() <= 1e-6 * thr
                    mism += int(bad.sum())
                    near += int((bad & close).sum())
                drawn_bad += int((~torch.isfinite(ours.gather(1, tok[:, None])).squeeze(1) & live).sum())
        res[mode] = {"n": n, "rejected_rows": rejected, "argmax_mismatch": argmax_bad, "scores_mismatch": mism,
                     "mismatch_near_threshold": near, "drawn_not_allowed": drawn_bad, "lp_abs": lp_worst, "widest_allowed": widest,
                     "finished_rows": int((seq == end[0]).any(1).sum()), "kept": kept, "total": total,
                     "first_ids": seq[:8, 0].tolist(),
                     "differs_from_plain": bool(seq.shape != plain[:, :n].shape or not torch.equal(seq, plain[:, :n]))}
    model._set_logits_processors(None)
    model._set_token_constraint(None)
    return res


def _ids(model, ids, mask, seqs, max_new, **kw):
    return model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=max_new, **kw).cpu()


def _launches(model):
    classes, _ = model.timing_names()
    return sum(int(model.timing_get(k)[1]) for k in classes)


def graphs(model, dev, B: int = 64, max_new: int = 16):
    """Off: the ids of a context that never saw a constraint, its own graph replayed, no launch of the new class.  On: a second
    call with another trie and other per-row starts instantiates no graph and changes the ids; one more launch per step."""
    cfg = model.cfg
    ids, mask, seqs = gsc.batch(cfg, B, seed=1)
    end = [cfg.dec_vocab - 3]
    out = {}
    fresh = model.new_context()
    p_fresh = _ids(fresh, ids, mask, seqs, max_new)
    del fresh
    p0 = _ids(model, ids, mask, seqs, max_new)
    i0 = model.stat("graph_instantiations")
    t1 = TokenTrie(big_members(2000, seed=3), end_token_id=end)
    a = _ids(model, ids, mask, seqs, max_new, eos_token_id=end, prefix_allowed_tokens_fn=t1)
    i1 = model.stat("graph_instantiations")
    rows = TokenTrie.per_row([TokenTrie(big_members(5 + b % 3, seed=100 + b), end_token_id=end) for b in range(B)])
    b_ = _ids(model, ids, mask, seqs, max_new, eos_token_id=end, prefix_allowed_tokens_fn=rows)
    i2 = model.stat("graph_instantiations")
    tab1, tabr = t1.compiled(), rows.compiled()
    r0 = model.stat("graph_replays")
    p1 = _ids(model, ids, mask, seqs, max_new)
    i3, r1 = model.stat("graph_instantiations"), model.stat("graph_replays")
    out.update(plain_equal_fresh=bool(torch.equal(p0, p_fresh)), plain_equal=bool(torch.equal(p0, p1)), on_graphs_first=i1 - i0,
               on_graphs_second=i2 - i1, plain_new_graphs=i3 - i2, plain_replays=r1 - r0,
               on_changed_ids=bool(a.shape != p0.shape or not torch.equal(a, p0)),
               second_changed_ids=bool(a.shape != b_.shape or not torch.equal(a, b_)),
               first_on_trie=all(_row_accepted(tab1, r, row, end[0]) for r, row in enumerate(a.tolist())),
               second_on_trie=all(_row_accepted(tabr, r, row, end[0]) for r, row in enumerate(b_.tolist())))
    model.timing(True)
    _ids(model, ids, mask, seqs, 4)
    off_cls, off_all = int(model.timing_get("constraint")[1]), _launches(model)
    model.timing(True)
    _ids(model, ids, mask, seqs, 4, prefix_allowed_tokens_fn=t1)          # (no eos: all 4 steps run)
    on = model.timing_get("constraint")
    on_all = _launches(model)
    model.timing(False)
    out.update(timing_off_launches=off_cls, timing_on_launches=int(on[1]), timing_on_ms=float(on[0]), all_launches_off=off_all,
               all_launches_on=on_all)
    model._set_token_constraint(None)
    return out


def _row_accepted(tab, r, row, end, pad=None) -> bool:
    """The row's ids up to its end id (if any) never leave the table; a finished row ended in a completing state and, with
    `pad`, holds only pads behind its end id."""
    body = row[: row.index(end)] if end in row else row
    s = tab.walk(r, body)
    if s == 0 or (end in row and not tab.completing[s]):
        return False
    return pad is None or end not in row or all(t == pad for t in row[row.index(end) + 1:])


def early_stop(model):
    """All rows reach their end id early: the call stops within 2 steps of the last row's end."""
    gp, ids, mask, seqs = _fixture()
    end, pad = int(gp["end"]), int(gp["pad"])
    res = {}
    for attempt in range(2):
        n0 = model.stat("decode_steps")
        o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, eos_token_id=[end], do_sample=False, max_new_tokens=16,
                           prefix_allowed_tokens_fn=fixture_fn(gp, "shared"))
        res[f"call{attempt}"] = {"n": int(o.shape[1]), "decode_steps": int(model.stat("decode_steps") - n0),
                                 "ids_equal": bool(np.array_equal(o.cpu().numpy(), gp["shared.sequences"]))}
    model._set_token_constraint(None)
    return res


def two_contexts(model, rounds: int = 4):
    """Two contexts with different tries in flight on two host threads: each follows its own (the fixture's ids)."""
    gp, ids, mask, seqs = _fixture()
    end, pad = int(gp["end"]), int(gp["pad"])
    other = model.new_context()
    got = {"shared": [], "per_row": []}

    def work(m, tag):
        fn = fixture_fn(gp, tag)
        for _ in range(rounds):
            o = m.generate(ids, seqs, attention_mask=mask, pad_token_id=pad, eos_token_id=[end], do_sample=False, max_new_tokens=16,
                           prefix_allowed_tokens_fn=fn)
            got[tag].append(o.cpu().numpy())
    th = [threading.Thread(target=work, args=(model, "shared")), threading.Thread(target=work, args=(other, "per_row"))]
    [t.start() for t in th]
    [t.join() for t in th]
    model._set_token_constraint(None)
    return {tag: all(np.array_equal(o, gp[tag + ".sequences"]) for o in got[tag]) and len(got[tag]) == rounds for tag in got}
