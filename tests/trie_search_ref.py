"""CPU twin of search_trie() (numpy): the level-synchronous beam search over a TokenTrie as OpusLlamaForCausalLM.search_trie's
docstring specifies it and as trie_beam_expand_kernel runs it.  Test infrastructure, not product code.

`expand_level` is one level for one prompt on a constraint.TrieSearchTable, with the edge log-probs and stop terms given by
callbacks (the kernel parity test hands it the device's own fp32 values); `search` loops it over a table of node log-probs and
stop terms per trie node - score_trie()'s node_logprobs row and per-node stop terms - and `brute_force` is the definition the
result is measured against: every member's exact path sum, sorted.

All score arithmetic is fp32 in the device's order: run' = run + lp, total = lp_member + stop."""
from __future__ import annotations

import numpy as np

F = np.float32
NEG = F(-np.inf)


def expand_level(tab, beams, pool, live, exhaustive, edge_lp, stop_lp, K, top, include_stop):
    """beams: K pairs (state, run) (state 0 or run -inf: dead); pool: at most `top` tuples (member, lp, stop), best first.
    edge_lp(k, e) -> fp32 log-prob of table edge e from beam k; stop_lp(k) -> fp32 stop term of beam k's state.
    Returns (beams', pool', live', exhaustive', tok [K], parent beam [K], edge lp [K], beam stop [K])."""
    beams = [(int(s), F(a)) if live and s > 0 and a > NEG else (0, NEG) for s, a in beams] + [(0, NEG)] * (K - len(beams))
    beam_stop = [NEG] * K
    offers = [(m, F(lp), F(st)) for m, lp, st in pool]
    cands = []                                              # (score, beam, edge)
    for k, (s, run) in enumerate(beams):
        if not s:
            continue
        if include_stop and tab.member[s] >= 0:
            st = F(stop_lp(k))
            beam_stop[k] = st
            if F(run + st) > NEG:
                offers.append((int(tab.member[s]), run, st))
        for e in range(int(tab.edge_off[s]), int(tab.edge_off[s + 1])):
            nx = int(tab.edge_next[e])
            sc = F(F(edge_lp(k, e)) + run)
            has_child = tab.edge_off[nx + 1] > tab.edge_off[nx]
            if not include_stop and tab.member[nx] >= 0 and sc > NEG:
                offers.append((int(tab.member[nx]), sc, F(0)))
            if include_stop or has_child:
                cands.append((sc, k, e))
    total = lambda o: F(o[1] + o[2])                        # noqa: E731
    offers.sort(key=lambda o: (-total(o), o[0]))            # descending, ties to the lower member index
    pool = offers[:top]
    need = total(pool[top - 1]) if len(pool) == top else NEG
    if len(cands) > K:
        exhaustive = False
    cands = [c for c in cands if c[0] > NEG]
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))           # descending, ties to the lower (beam, id): edges ascend in id
    cands = cands[:K]
    live = bool(cands) and not cands[0][0] < need
    if not live:
        cands = []
    new, tok, par, elp = [], [], [], []
    for j in range(K):
        if j < len(cands):
            sc, k, e = cands[j]
            new.append((int(tab.edge_next[e]), sc))
            tok.append(int(tab.edge_tok[e]))
            par.append(k)
            elp.append(F(edge_lp(k, e)))
        else:
            new.append((0, NEG))
            tok.append(0)
            par.append(j)
            elp.append(NEG)
    return new, pool, live, exhaustive, tok, par, elp, beam_stop


def search(tab, p, node_lp, stop_node, K, top, prune=True):
    """The whole search for prompt p: node_lp [nodes] fp32 per trie node (node = state - root), stop_node likewise or None
    (no stop term).  prune=False keeps going until no beam is left (the test of the pruning rule).  Returns a dict: member_index /
    logprob / member_logprob / stop_logprob [top] (-1 / -inf padding), levels, exhaustive, trace (per level the new beams' (node,
    edge lp, run))."""
    root = int(tab.start[p])
    include_stop = stop_node is not None
    keep = top if prune else 1 << 30                         # (no pruning: the pool is never full, cut in the result only)
    beams, pool, live, exhaustive, levels, trace = [(root, F(0))], [], True, True, 0, []
    for _ in range(tab.max_depth + 2):
        if not live:
            break
        cur = beams
        beams, pool, live, exhaustive, _, _, elp, _ = expand_level(
            tab, cur, pool, True, exhaustive, lambda k, e: node_lp[int(tab.edge_next[e]) - root],
            lambda k: stop_node[cur[k][0] - root], K, keep, include_stop)
        levels += 1
        trace.append([(s - root, float(l), float(a)) for (s, a), l in zip(beams, elp) if s])
    assert not live, "the trie's depth bounds the search"
    out = dict(member_index=np.full(top, -1, np.int64), logprob=np.full(top, NEG), member_logprob=np.full(top, NEG),
               stop_logprob=np.full(top, NEG) if include_stop else None, levels=levels, exhaustive=exhaustive, trace=trace)
    for r, (m, lp, st) in enumerate(pool[:top]):
        out["member_index"][r], out["member_logprob"][r], out["logprob"][r] = m, lp, F(lp + st)
        if include_stop:
            out["stop_logprob"][r] = st
    return out


def brute_force(trie, node_lp, stop_node, top):
    """Every member's exact score by definition: the path's node log-probs added in fp32 from the root, + the stop term at its
    node; the best `top` (descending, ties to the lower member index) as (member_index, logprob, member_logprob, stop_logprob)."""
    rows = []
    for m, node in enumerate(trie.member_nodes):
        path, v = [], node
        while v:
            path.append(v)
            v = trie.node_par[v]
        acc = F(0)
        for v in path[::-1]:
            acc = F(acc + F(node_lp[v]))
        st = F(stop_node[node]) if stop_node is not None else F(0)
        rows.append((m, F(acc + st), acc, st))
    rows.sort(key=lambda r: (-r[1], r[0]))
    rows = rows[:top]
    idx = np.full(top, -1, np.int64)
    tot, lp, st = np.full(top, NEG), np.full(top, NEG), np.full(top, NEG)
    for r, (m, t, a, s) in enumerate(rows):
        idx[r], tot[r], lp[r], st[r] = m, t, a, s
    return idx, tot, lp, st
