"""Checks of trie scoring (OpusLlamaForCausalLM.score_trie) shared by tests/test_gpu_trie_score.py and its bf16 child
tests/bf16_trie_score_check.py: each returns a dict of observations; the callers assert the bounds of their build.
Test infrastructure, not product code."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.constraint import TRIE_MAX_DEPTH, TokenTrie, plan_trie_score
import forward_checks as fc
import prefix_checks as pc

GOLD = fc.GOLD
END = 1


# ------------------------------------------------------------------------------------------------ the attention kernel alone
KERNEL_SHAPES = [            # (head_dim, heads, kv heads): GQA 4 and MHA at head dims 64 / 128, the small head dims once
    (64, 4, 1), (64, 4, 4), (128, 8, 2), (128, 4, 4), (16, 4, 2), (32, 6, 2),
]


def _forest(rng, P, kind, G):
    """Rows (src, par, depth) of a pass: parents earlier, same prefix row, one level up."""
    src, par, depth = [], [], []

    def add(p, q):
        src.append(p)
        par.append(q)
        depth.append(1 if q < 0 else depth[q] + 1)
        return len(src) - 1

    if kind == "depth1":                                   # children of the root only
        for p in range(P):
            for _ in range(1 + 2 * p):
                add(p, -1)
    elif kind == "chain":                                  # one path down to the depth limit per prefix row
        for p in range(P):
            q = -1
            for _ in range(TRIE_MAX_DEPTH if p != 1 else 3):
                q = add(p, q)
    else:                                                  # random trees, each crossing a block of 128 stacked queries
        per = [128 // G + 9, 3, 2 * (128 // G) + 5][:P]
        if kind == "per_row":
            per = [5, 128 // G + 1, 40][:P]
        mine = [[] for _ in range(P)]
        order = np.concatenate([np.full(n, p) for p, n in enumerate(per)])
        rng.shuffle(order)                                 # the rows of the prefix rows interleave
        for p in order.tolist():
            cand = [q for q in mine[p] if depth[q] < TRIE_MAX_DEPTH]
            q = -1 if not cand or rng.random() < 0.2 else int(rng.choice(cand))
            mine[p].append(add(p, q))
    return np.asarray(src, np.int32), np.asarray(par, np.int32), np.asarray(depth, np.int32)


def _tree_ref(q, kh, vh, kn, vn, kstart, src, par, G):
    """fp64: q [R, nh, hd], kh / vh [P, nkv, Tp, hd], kn / vn [R, nkv, hd] -> [R, nh hd]."""
    R, nh, hd = q.shape
    out = torch.empty((R, nh, hd), dtype=torch.float64)
    for r in range(R):
        p = int(src[r])
        chain, a = [], r
        while a >= 0:
            chain.append(a)
            a = int(par[a])
        K = torch.cat([kh[p, :, int(kstart[p]):], kn[chain].transpose(0, 1)], 1).repeat_interleave(G, 0)      # [nh, L + d, hd]
        V = torch.cat([vh[p, :, int(kstart[p]):], vn[chain].transpose(0, 1)], 1).repeat_interleave(G, 0)
        s = torch.einsum("hd,hjd->hj", q[r], K) * hd ** -0.5
        out[r] = torch.einsum("hj,hjd->hd", torch.softmax(s, -1), V)
    return out.reshape(R, nh * hd)


def attn_kernel(dev) -> dict:
    """opus_debug_attn_tree against fp64 on the same operands: every KERNEL_SHAPES x (random trees whose stacked queries cross a
    128-query block, per-row trees, depth 1 only, chains of the depth limit), prefix rows with kstart 0, > 32 and Tp - 1; the
    worst absolute error per shape."""
    dt = _cabi.operand_dtype()
    lib = _cabi.lib()
    obs = {}
    for hd, nh, nkv in KERNEL_SHAPES:
        cfg = opa.micro(dec_dim=max(64, nh * hd), dec_heads=nh, dec_kv_heads=nkv, dec_head_dim=hd, max_prompt=160, max_batch=4)
        model = fc.make_model(cfg, dev)
        G = nh // nkv
        worst = 0.0
        for k, kind in enumerate(("random", "per_row", "depth1", "chain")):
            rng = np.random.default_rng(hd * 100 + nh * 10 + k)
            gen = torch.Generator().manual_seed(hd * 1000 + nh * 10 + k)
            P = 3
            Tp = cfg.max_prompt if k % 2 else 77
            kstart = torch.tensor([0, 41, Tp - 1], dtype=torch.int32)                  # (0, > 32, a row of one real slot)
            src, par, depth = _forest(rng, P, kind, G)
            R = len(src)
            QKV = (nh + 2 * nkv) * hd
            qkv = torch.randn(R, QKV, generator=gen).to(dt)
            kh = torch.randn(P, nkv, Tp, hd, generator=gen).to(dt)
            vh = torch.randn(P, nkv, Tp, hd, generator=gen).to(dt)
            q = qkv[:, : nh * hd].double().view(R, nh, hd)
            kn = qkv[:, nh * hd: (nh + nkv) * hd].double().view(R, nkv, hd)
            vn = qkv[:, (nh + nkv) * hd:].double().view(R, nkv, hd)
            ref = _tree_ref(q, kh.double(), vh.double(), kn, vn, kstart, src, par, G)
            d = lambda t: t.contiguous().to(dev)                                       # noqa: E731
            out = torch.zeros(R, nh * hd, dtype=dt, device=dev)
            dq, dk, dv, dks = d(qkv), d(kh), d(vh), d(kstart)
            _cabi.check(lib.opus_debug_attn_tree(model._ctx, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dks.data_ptr(), P, Tp, R,
                                                 src.ctypes.data, par.ctypes.data, depth.ctypes.data, out.data_ptr(), None))
            torch.cuda.synchronize()
            worst = max(worst, float((out.double().cpu() - ref).abs().max()))
        obs[f"hd{hd}_g{G}"] = worst
        del model
    return obs


# ------------------------------------------------------------------------------------------------ the reference's forward
def golden_spans(dev) -> dict:
    """Rows of tests/golden/forward_micro.npz (the reference's own forward), split at their first counted label as
    prefix_checks.golden_split does: the prompt in front is the prefix, the labelled span behind it a ONE-member trie of its own
    (TokenTrie.per_row).  The node log-probs of the path against the fixture's token log-probs, with proteins (a) and without (c)."""
    cfg = opa.micro()
    model = fc.make_model(cfg, dev)
    g = np.load(os.path.join(GOLD, "forward_micro.npz"))
    seqs = json.load(open(os.path.join(GOLD, "forward_micro.seqs.json")))
    obs = {}
    for tag in "ac":
        ids, mask, lab = g[tag + ".ids"], g[tag + ".mask"].astype(bool), g[tag + ".labels"]
        B = ids.shape[0]
        pre, tries, want = [], [], []
        for b in range(B):
            real = np.flatnonzero(mask[b])
            t0 = int(np.flatnonzero(lab[b] != -100)[0])
            pre.append(ids[b, real[real < t0]])
            tail = real[real >= t0]
            member = ids[b, tail].astype(np.int64).tolist()
            end = next(t for t in range(cfg.dec_vocab) if t not in member)              # (an end id outside the member)
            tries.append(TokenTrie([member], end_token_id=END if END not in member else end))
            counted = lab[b, tail] != -100
            want.append((counted, g[tag + ".token_logprobs"][b][g[tag + ".labels_out"][b] != -100]))
        ends = {tuple(t.end_ids) for t in tries}
        assert len(ends) == 1, ends
        T = max(len(p) for p in pre)
        pids = np.full((B, T), 2, dtype=np.int64)
        pm = np.zeros((B, T), dtype=bool)
        for b, p in enumerate(pre):
            pids[b, T - len(p):] = p
            pm[b, T - len(p):] = True
        kw = dict(seq=seqs) if bool(g[tag + ".has_seq"]) else {}
        prefix = model.cache_prefix(torch.from_numpy(pids), attention_mask=torch.from_numpy(pm), **kw)
        res = model.score_trie(prefix, TokenTrie.per_row(tries))
        err = 0.0
        for b, (counted, ref_row) in enumerate(want):
            n = tries[b].n_nodes                                                        # one member: node j + 1 = its token j
            got = res.node_logprobs[b, 1: n + 1].double().cpu()[torch.from_numpy(counted)]
            assert got.numel() == ref_row.size
            err = max(err, float((got - torch.from_numpy(ref_row)).abs().max()))
            assert bool((res.node_logprobs[b, n + 1:] == 0).all())                       # (a shorter span's padding)
        obs[tag] = err
    del model
    return obs


# ------------------------------------------------------------------------------------------------ oracle and the flat call
def random_trie(rng, n, lo=1, hi=5, alphabet=10, separator=None, first=3):
    """n members over a small alphabet (shared prefixes); one is a prefix of another unless a separator forbids nothing here."""
    members = [rng.integers(first, first + alphabet, int(rng.integers(lo, hi + 1))).tolist() for _ in range(n)]
    if n >= 2 and len(members[0]) > 1:
        members[1] = members[0][:-1]                                                   # a member that is a prefix of another
    return TokenTrie(members, end_token_id=END, separator=separator)


def _oracle(cfg, dev, prompts, tries):
    """fp32 oracle on the concatenated rows prompt + member: per (p, node) the log-prob of the node's token, per (p, member)
    the log of the stop ids' probability mass behind the member."""
    import oracle
    W = fc.Canon32(cfg, dev)
    rows, who = [], []
    for p, t in enumerate(tries):
        for m, ids in enumerate(t.member_ids):
            rows.append(np.concatenate([prompts[p], np.asarray(ids, dtype=np.int64)]))
            who.append((p, m))
    T = max(len(r) for r in rows)
    f = oracle.opt_forward if cfg.dec_arch == 1 else oracle.llama_forward
    N = max(t.n_nodes for t in tries)
    M = max(len(t.member_ids) for t in tries)
    node = torch.zeros((len(tries), N + 1), dtype=torch.float64)
    stop = torch.full((len(tries), M), float("-inf"), dtype=torch.float64)
    step = 8                                                                           # rows per oracle call (its logits are [R, T, V])
    for r0 in range(0, len(rows), step):
        chunk = rows[r0: r0 + step]
        cids = torch.full((len(chunk), T), 2, dtype=torch.long)
        cmask = torch.zeros((len(chunk), T), dtype=torch.bool)
        for r, row in enumerate(chunk):
            cids[r, : len(row)] = torch.from_numpy(row)
            cmask[r, : len(row)] = True
        with torch.no_grad():
            logits, _ = f(W["dec.embed_tokens"][cids], cmask, W, cfg, all_logits=True)
        lsm = torch.log_softmax(logits.double(), dim=-1)
        for r, row in enumerate(chunk):
            p, m = who[r0 + r]
            t, a, v = tries[p], len(prompts[p]), 0
            for j, tok in enumerate(t.member_ids[m]):
                v = t.children[v][tok]
                node[p, v] = lsm[r, a + j - 1, tok]
            stop[p, m] = torch.logsumexp(lsm[r, len(row) - 1, torch.tensor(t.stop_ids())], 0)
    return node, stop


def vs_oracle(dev, cfg, P, sizes, seed=0, per_row=False, oracle_check=True, hi=5, model=None) -> dict:
    """score_trie on random tries with shared prefixes behind P left-padded prompts: node log-probs and stop terms against the
    fp32 oracle on the concatenated rows and against score_continuations on the flat member list (same prefix handle);
    include_stop False / True against each other; the same call twice; the definitions of member_logprob / logprob / topk;
    the padding of per-row tries; rows_evaluated against the plan."""
    model = model or fc.make_model(cfg, dev)
    rng = np.random.default_rng(seed)
    prompts, _, ids, mask = pc._prefix_batch(cfg, P, 1, seed)
    if per_row:
        tries = [random_trie(rng, int(n), hi=hi, separator=[20, 21] if k == 0 else None) for k, n in zip(range(P), sizes)]
        trie = TokenTrie.per_row(tries)
    else:
        trie = random_trie(rng, int(sizes[0]), hi=hi)
        tries = [trie] * P
    prefix = model.cache_prefix(ids, attention_mask=mask)
    full = model.score_trie(prefix, trie, include_stop=True)
    full2 = model.score_trie(prefix, trie, include_stop=True)
    bare = model.score_trie(prefix, trie)
    bare2 = model.score_trie(prefix, trie)
    # the flat call on every member of every prompt
    conts, src = [], []
    for p, t in enumerate(tries):
        conts += [torch.tensor(m, dtype=torch.long) for m in t.member_ids]
        src += [p] * len(t.member_ids)
    flat = model.score_continuations(prefix, conts, prefix_rows=torch.tensor(src))
    again = model.score_trie(prefix, trie, include_stop=True)                            # (the flat call leaves the handle valid)
    N, M = full.node_logprobs.shape[1] - 1, full.member_logprob.shape[1]
    flat_node = torch.zeros((P, N + 1), dtype=torch.float64)
    seen = torch.zeros((P, N + 1), dtype=torch.bool)
    r = 0
    for p, t in enumerate(tries):
        for m in t.member_ids:
            v = 0
            for j, tok in enumerate(m):
                v = t.children[v][tok]
                flat_node[p, v] = float(flat.token_logprobs[r, j])
                seen[p, v] = True
            r += 1
    real = torch.zeros((P, N + 1), dtype=torch.bool)
    realm = torch.zeros((P, M), dtype=torch.bool)
    for p, t in enumerate(tries):
        real[p, 1: t.n_nodes + 1] = True
        realm[p, : len(t.member_ids)] = True
    assert torch.equal(seen, real)
    got = full.node_logprobs.double().cpu()
    # member_logprob by its definition: the path's node log-probs added in fp32 from the root to the leaf
    want_member = torch.full((P, M), float("-inf"))
    nl = full.node_logprobs.cpu()
    for p, t in enumerate(tries):
        for m, node in enumerate(t.member_nodes):
            path, v = [], node
            while v:
                path.append(v)
                v = t.node_par[v]
            acc = torch.zeros((), dtype=torch.float32)
            for v in path[::-1]:
                acc = acc + nl[p, v]
            want_member[p, m] = acc
    k = min(3, M)
    vals, idx = full.topk(k)
    plan_full = plan_trie_score(tries, True, 10 ** 9)
    plan_bare = plan_trie_score(tries, False, 10 ** 9)
    obs = dict(
        P=P, N=N, M=M, rows_full=full.rows_evaluated, rows_bare=bare.rows_evaluated,
        flat_abs=float((got - flat_node)[real].abs().max()),
        stop_modes_abs=float((full.node_logprobs - bare.node_logprobs).abs().max()),
        bitwise=bool(torch.equal(full.node_logprobs, full2.node_logprobs) and torch.equal(full.stop_logprob, full2.stop_logprob)
                     and torch.equal(full.member_logprob, full2.member_logprob) and torch.equal(bare.node_logprobs, bare2.node_logprobs)
                     and torch.equal(bare.member_logprob, bare2.member_logprob) and torch.equal(full.logprob, again.logprob)),
        member_def=bool(torch.equal(full.member_logprob.cpu(), want_member)),
        logprob_def=bool(torch.equal(full.logprob, full.member_logprob + full.stop_logprob) and bare.stop_logprob is None
                         and torch.equal(bare.logprob, bare.member_logprob)),
        root_zero=bool((full.node_logprobs[:, 0] == 0).all()),
        pad_ok=bool((got[~real] == 0).all() and (full.member_logprob.cpu()[~realm] == float("-inf")).all()
                    and (full.stop_logprob.cpu()[~realm] == float("-inf")).all() and (full.logprob.cpu()[~realm] == float("-inf")).all()
                    and torch.isfinite(full.logprob.cpu()[realm]).all()
                    and full.n_members.cpu().tolist() == [len(t.member_ids) for t in tries]),
        topk_ok=bool(torch.equal(vals, torch.topk(full.logprob, k, dim=1).values) and torch.equal(full.logprob.gather(1, idx), vals)),
        rows_ok=bool(full.rows_evaluated >= plan_full.evaluated_nodes and bare.rows_evaluated >= plan_bare.evaluated_nodes),
        one_pass_rows=[plan_full.evaluated_nodes, plan_bare.evaluated_nodes],
    )
    if oracle_check:
        node, stop = _oracle(cfg, dev, prompts, tries)
        obs["oracle_abs"] = float((got - node)[real].abs().max())
        obs["stop_abs"] = float((full.stop_logprob.double().cpu() - stop)[realm].abs().max())
    return obs
