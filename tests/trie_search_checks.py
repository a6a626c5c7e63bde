"""Checks of trie search (OpusLlamaForCausalLM.search_trie) shared by tests/test_gpu_trie_search.py and its bf16 child
tests/bf16_trie_search_check.py: each returns a dict of observations; the callers assert the bounds of their build.
Test infrastructure, not product code."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TokenTrie, TrieSearchTable
import forward_checks as fc
import prefix_checks as pc
import trie_search_ref as ref

END = 1
F = np.float32


# ------------------------------------------------------------------------------------------------ the expand kernel alone
def kernel_tries(rng, V, P):
    """P tries for the kernel test (TokenTrie.per_row starts): a wide one (V >= 8192: a root of more than 4 096 children, some of
    them members with children, some leaves), random ones with shared prefixes, a chain (states with one child) and a one-member
    trie."""
    ids = np.arange(3, V)
    out = []
    for p in range(P):
        kind = p % 4
        if kind == 0:
            n = 5000 if V >= 8192 else 40
            first = rng.choice(ids, size=n, replace=False).tolist()
            members = [[t] for t in first[: n // 2]]                                        # leaves below the root
            for t in first[n // 2:]:
                members += [[t, int(x)] for x in rng.choice(ids, size=2, replace=False)]
            members += [[t] for t in first[n // 2: n // 2 + n // 8]]                         # members that have children
            out.append(TokenTrie(members, END))
        elif kind == 1:
            a = ids[: 12]
            members = [rng.choice(a, size=int(rng.integers(1, 6))).tolist() for _ in range(60)]
            members[1] = members[0][:-1] or members[1]
            out.append(TokenTrie(members, END, separator=[2, int(ids[-1])]))
        elif kind == 2:
            out.append(TokenTrie([[int(t) for t in rng.choice(ids, size=6, replace=False)]], END))   # a chain: one child per state
        else:
            out.append(TokenTrie([[int(ids[5])]], END))
    return out


def expand_kernel(model, V, P, K, seed) -> dict:
    """opus_debug_trie_beam_expand on caller logits [P K, V] (and, first level, [P, V]) against trie_search_ref.expand_level fed
    the device's own log-sum-exp: ids, parent rows, states, member indices and flags exact, scores and edge log-probs bitwise, no
    NaN, the logits untouched.  Logits and running scores lie on a grid of 1/4, so that equal scores are common; beams stand on
    the root (the wide fan-out), on leaves (no child), on chain states (one child), on member states with children; some are
    dead; pools start empty, partly filled and full."""
    dev = model.device
    lib = _cabi.lib()
    rng = np.random.default_rng(seed)
    tries = kernel_tries(rng, V, P)
    tab = TrieSearchTable(tries)
    p_ = lambda a: a.ctypes.data                                                             # noqa: E731
    _cabi.check(lib.opus_set_trie_search(model._ctx, tab.n_states, p_(tab.edge_off), p_(tab.edge_tok), p_(tab.edge_next), tab.n_edges,
                                         p_(tab.member), p_(tab.stop_set), len(tab.stop_off) - 1, p_(tab.stop_off), p_(tab.stop_ids), None))
    obs = dict(V=V, P=P, K=K, launches=0, ties=0, wide_states=0, dead=0, stop_abs=0.0, ok=True, why=[])

    def fail(msg):
        obs["ok"] = False
        obs["why"].append(msg)

    for first in (True, False):
        for stop in (False, True):
            top = max(1, min(K, 3 if stop else K))
            rows = P if first else P * K
            logits = (rng.integers(-24, 25, size=(rows, V)).astype(F) / F(4))
            state = np.zeros((P, K), np.int32)
            score = np.full((P, K), -np.inf, F)
            pool_m = np.full((P, top), -1, np.int32)
            pool_lp = np.full((P, top), -np.inf, F)
            pool_st = np.full((P, top), -np.inf, F)
            for p, t in enumerate(tries):
                root = int(tab.start[p])
                if first:
                    state[p, 0], score[p, 0] = root, 0
                else:
                    nodes = rng.permutation(len(t.children))[:K]
                    if p % 4 == 0:
                        nodes[0] = 0                                                         # the wide root
                    for k, n in enumerate(nodes.tolist()):
                        state[p, k] = root + n
                        score[p, k] = -F(rng.integers(0, 12)) / F(4)
                    if K > 1:
                        dead = rng.integers(1, K)                                            # (beam 0 stays: the wide root)
                        if rng.random() < 0.5:
                            state[p, dead] = 0                                               # dead by its state ...
                        else:
                            score[p, dead] = -np.inf                                         # ... or by its score
                    obs["dead"] += int(((state[p] == 0) | ~(score[p] > -np.inf)).sum())
                fill = (0, top // 2, top)[p % 3]                                             # the pool as earlier levels left it
                for r in range(fill):
                    pool_m[p, r] = 10 ** 6 + 7 * p + (top - r)                               # (descending totals, ties by index)
                    pool_lp[p, r] = -F(1 + (r // 2)) / F(2)
                    pool_st[p, r] = -F(0.25) if stop else 0
            flags = np.tile(np.asarray([1, 1, 0], np.int32), (P, 1))
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                  # noqa: E731
            d_logits, d_state, d_score = d(logits), d(state), d(score)
            before = d_logits.clone()
            d_pm, d_pl, d_ps, d_flags = d(pool_m), d(pool_lp), d(pool_st), d(flags)
            i32 = dict(dtype=torch.int32, device=dev)
            d_tok, d_par, d_words = torch.full((P * K,), -7, **i32), torch.full((P * K,), -7, **i32), torch.full((2,), -7, **i32)
            d_lse = torch.zeros((P * K,), dtype=torch.float32, device=dev)
            d_elp = torch.full((P, K), float("nan"), device=dev)
            d_bst = torch.full((P, K), float("nan"), device=dev)
            io = _cabi.CTrieSearchIO(P, K, top, int(stop), d_state.data_ptr(), d_score.data_ptr(), d_tok.data_ptr(), d_par.data_ptr(),
                                     d_pm.data_ptr(), d_pl.data_ptr(), d_ps.data_ptr(), d_flags.data_ptr(), d_words.data_ptr(),
                                     d_lse.data_ptr(), d_elp.data_ptr(), d_bst.data_ptr())
            _cabi.check(lib.opus_debug_trie_beam_expand(model._ctx, d_logits.data_ptr(), V, C.byref(io), int(first), None))
            torch.cuda.synchronize()
            obs["launches"] += 1
            if not torch.equal(before, d_logits):
                fail("the logits changed")
            lse = d_lse.cpu().numpy()
            want_lse = torch.logsumexp(torch.from_numpy(logits).double(), 1).numpy()
            if np.abs(lse[:rows] - want_lse).max() > 1e-4:
                fail("log-sum-exp off")
            g_state, g_score = d_state.cpu().numpy(), d_score.cpu().numpy()
            g_tok, g_par = d_tok.cpu().numpy().reshape(P, K), d_par.cpu().numpy().reshape(P, K)
            g_elp, g_bst = d_elp.cpu().numpy(), d_bst.cpu().numpy()
            g_pm, g_pl, g_ps, g_flags = d_pm.cpu().numpy(), d_pl.cpu().numpy(), d_ps.cpu().numpy(), d_flags.cpu().numpy()
            for name, a in (("score", g_score), ("edge_lp", g_elp), ("beam_stop", g_bst), ("pool_lp", g_pl), ("pool_stop", g_ps)):
                if np.isnan(a).any():
                    fail("NaN in " + name)
            bits = lambda a: np.asarray(a, F).view(np.int32)                                 # noqa: E731
            live_n = moved_n = 0
            for p, t in enumerate(tries):
                row = (lambda k: p) if first else (lambda k: p * K + k)                      # noqa: E731
                elp = lambda k, e: F(logits[row(k), tab.edge_tok[e]]) - F(lse[row(k)])       # noqa: E731
                old = [(int(m), F(a), F(s)) for m, a, s in zip(pool_m[p], pool_lp[p], pool_st[p]) if m >= 0]
                beams = list(zip(state[p].tolist(), score[p].tolist()))
                new, pool, live, exh, tok, par, e_lp, _ = ref.expand_level(tab, beams, old, True, True, elp, lambda k: g_bst[p, k], K, top, stop)
                if stop:                                                                    # the stop terms the twin took from the device
                    for k, (s, a) in enumerate(beams):
                        alive = s > 0 and a > -np.inf
                        if alive and tab.member[s] >= 0:
                            ids = tab.stop_ids[tab.stop_off[tab.stop_set[s]]: tab.stop_off[tab.stop_set[s] + 1]]
                            want = float(torch.logsumexp(torch.from_numpy(logits[row(k), ids]).double(), 0)) - float(want_lse[row(k)])
                            obs["stop_abs"] = max(obs["stop_abs"], abs(float(g_bst[p, k]) - want))
                        elif g_bst[p, k] != -np.inf:
                            fail("a stop term for a beam that is on no member")
                elif not (g_bst[p] == -np.inf).all():
                    fail("stop terms without include_stop")
                sc = [a for _, a in new]
                obs["ties"] += int(sum(1 for j in range(K - 1) if sc[j] == sc[j + 1] and sc[j] > -np.inf))
                obs["wide_states"] += int(sum(1 for s, a in beams if s > 0 and a > -np.inf and tab.edge_off[s + 1] - tab.edge_off[s] > 4096))
                if g_tok[p].tolist() != tok or g_par[p].tolist() != [p * K + k for k in par] or g_state[p].tolist() != [s for s, _ in new]:
                    fail(f"ids / parents / states of prompt {p} (first={first} stop={stop})")
                if not np.array_equal(bits(g_score[p]), bits(sc)) or not np.array_equal(bits(g_elp[p]), bits(e_lp)):
                    fail(f"scores of prompt {p} not bitwise (first={first} stop={stop})")
                w_m = [m for m, _, _ in pool] + [-1] * (top - len(pool))
                w_lp = [a for _, a, _ in pool] + [-np.inf] * (top - len(pool))
                w_st = [s for _, _, s in pool] + [-np.inf] * (top - len(pool))
                if g_pm[p].tolist() != w_m or not np.array_equal(bits(g_pl[p]), bits(w_lp)) or not np.array_equal(bits(g_ps[p]), bits(w_st)):
                    fail(f"pool of prompt {p} (first={first} stop={stop})")
                moved = any(q != k for k, q in enumerate(par))
                if g_flags[p].tolist() != [int(live), int(exh), int(moved)]:
                    fail(f"flags of prompt {p}: {g_flags[p].tolist()} for {[int(live), int(exh), int(moved)]}")
                live_n += int(live)
                moved_n += int(moved)
                if ((g_tok[p] < 0) | (g_tok[p] >= V)).any():
                    fail("an id outside the vocabulary")
            if d_words.cpu().tolist() != [live_n, moved_n]:
                fail("summary words")
    return obs


# ------------------------------------------------------------------------------------------------ end to end against score_trie
def node_stop_table(trie, sc, p):
    """score_trie's stop terms of prompt p per trie node (-inf where the node completes no member)."""
    st = np.full(trie.n_nodes + 1, -np.inf, F)
    row = sc.stop_logprob[p].cpu().numpy()
    for m, node in enumerate(trie.member_nodes):
        st[node] = row[m]
    return st


def decisive_ranks(vals, margin):
    """Ranks of a descending list whose neighbours both differ from it by more than `margin` (-inf padding counts as far)."""
    out = []
    for r, v in enumerate(vals):
        lo = r == 0 or vals[r - 1] - v > margin
        hi = r + 1 == len(vals) or v - vals[r + 1] > margin or vals[r + 1] == -np.inf
        out.append(bool(lo and hi and v > -np.inf))
    return out


def vs_score_trie(model, cfg, P, tries, K, top, stop, seed, alone, per_row=False, prefix=None, ids_mask=None) -> dict:
    """search_trie(return_trace=True) against score_trie on the same prefix and trie: every beam of every level per NODE (edge
    log-prob against node_logprobs, stop terms against stop_logprob); the twin on score_trie's own table has to name the device's
    members at every rank whose neighbours in that table lie further than 2 x depth x `alone` away; an exhaustive row against
    score_trie(...).topk(top) by the same rule; the call twice: bitwise."""
    trie = TokenTrie.per_row(tries) if per_row else tries[0]
    if prefix is None:
        _, _, ids, mask = ids_mask if ids_mask is not None else pc._prefix_batch(cfg, P, 1, seed)
        prefix = model.cache_prefix(ids, attention_mask=mask, detach=True)
    sc = model.score_trie(prefix, trie, include_stop=stop)
    res = model.search_trie(prefix, trie, num_beams=K, top=top, include_stop=stop, return_trace=True)
    res2 = model.search_trie(prefix, trie, num_beams=K, top=top, include_stop=stop)
    tab = TrieSearchTable(tries)
    node_lp = sc.node_logprobs.cpu().numpy()
    depth = max(t.max_depth for t in tries)
    margin = 2 * depth * alone
    obs = dict(P=P, K=K, top=top, stop=stop, levels=res.levels, rows_decoded=res.rows_decoded, rows_score_trie=sc.rows_evaluated,
               exhaustive=res.exhaustive.cpu().tolist(), node_abs=0.0, stop_abs=0.0, beams_compared=0, stops_compared=0,
               ranks=0, decisive=0, rank_mismatch=0, topk_mismatch=0, twin_exhaustive_same=True, pad_ok=True, sorted_ok=True)
    obs["bitwise"] = bool(torch.equal(res.member_index, res2.member_index) and torch.equal(res.logprob, res2.logprob)
                          and torch.equal(res.exhaustive, res2.exhaustive) and res.levels == res2.levels and res2.trace is None)
    obs["no_nan"] = not bool(torch.isnan(res.logprob).any() or torch.isnan(res.member_logprob).any())
    stop_tables = [node_stop_table(tries[p], sc, p) if stop else None for p in range(P)]
    for lv in res.trace:
        for j in range(len(lv["prompt"])):
            p = int(lv["prompt"][j])
            if bool(lv["alive"][j]):
                obs["node_abs"] = max(obs["node_abs"], abs(float(lv["edge_logprob"][j]) - float(node_lp[p, int(lv["node"][j])])))
                obs["beams_compared"] += 1
            if stop and bool(lv["from_alive"][j]) and float(lv["from_stop"][j]) > -np.inf:
                obs["stop_abs"] = max(obs["stop_abs"], abs(float(lv["from_stop"][j]) - float(stop_tables[p][int(lv["from_node"][j])])))
                obs["stops_compared"] += 1
    got_idx, got_lp = res.member_index.cpu().numpy(), res.logprob.cpu().numpy()
    full = sc.logprob.cpu().numpy()
    for p in range(P):
        tw = ref.search(tab, p, node_lp[p], stop_tables[p], K, top)
        dec = decisive_ranks(tw["logprob"].tolist(), margin)
        n_mem = len(tries[p].member_ids)
        for r in range(top):
            if tw["member_index"][r] < 0:
                continue
            obs["ranks"] += 1
            obs["decisive"] += int(dec[r])
            if dec[r] and got_idx[p, r] != tw["member_index"][r]:
                obs["rank_mismatch"] += 1
        if bool(res.exhaustive[p]) != tw["exhaustive"]:
            obs["twin_exhaustive_same"] = False
        if bool(res.exhaustive[p]):                                                         # then it is score_trie's top-k
            order = sorted(range(n_mem), key=lambda m: (-full[p, m], m))[:top]
            vals = [float(full[p, m]) for m in order]
            dec = decisive_ranks(vals + [-np.inf] * (top - len(vals)), margin)
            for r, m in enumerate(order):
                if dec[r] and got_idx[p, r] != m:
                    obs["topk_mismatch"] += 1
        found = got_idx[p] >= 0
        n_found = int(found.sum())
        if not (found[:n_found].all() and (got_lp[p, n_found:] == -np.inf).all() and n_found == min(top, n_found)
                and (n_found == min(top, n_mem) or not bool(res.exhaustive[p]))):
            obs["pad_ok"] = False
        if n_found > 1 and not (np.diff(got_lp[p, :n_found]) <= 0).all():
            obs["sorted_ok"] = False
    return obs, res, sc
