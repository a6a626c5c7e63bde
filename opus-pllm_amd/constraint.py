"""Constrained decoding: a trie of allowed answers as generate()'s `prefix_allowed_tokens_fn`.

    trie = TokenTrie(sequences, end_token_id=eos)                      # one member of a closed vocabulary, then an end id
    trie = TokenTrie(sequences, end_token_id=eos, separator=[ids])     # a list: "m1 sep m2 sep m3 <end>"
    rows = TokenTrie.per_row([trie_0, trie_1, ...])                    # row b follows trie_b
    out = model.generate(ids, seqs, ..., eos_token_id=eos, prefix_allowed_tokens_fn=trie)

The object is a plain transformers callback, `trie(batch_id, sent) -> sorted list of allowed ids` (what
PrefixConstrainedLogitsProcessor calls per row and step, `sent` = the ids generated so far), and that callback is the definition
of the feature.  On the GPU it never runs: the object compiles itself once to a deterministic automaton in CSR form
(`compiled()`), generate() uploads the table, and a kernel in the captured decode step keeps one state word per row and writes
-inf outside the state's allowed set.

Semantics, walking `sent` from the row's root:
  * in a trie state the allowed ids are the children's ids; in a state that completes a member, also every end id and, with a
    separator, the separator's first id (its ids lead back to the root: any number of members, each any number of times);
  * after an end id, and after any id that was not allowed (a finished row's pads), the allowed ids are the end ids - never an
    empty list.
Rows finish at an end id only if the caller passes the same ids as generate()'s `eos_token_id`.  A row whose every allowed id was
banned by another processor (min_new_tokens larger than its shortest member, a bad word) is the caller's error.

The same object is what OpusLlamaForCausalLM.score_trie(prefix, trie) scores: exact log-probabilities of EVERY member behind a
cached prompt in one tree pass.  For that a trie numbers its members (`member_ids`, `member_nodes`, `input_member`,
`member_strings`) and `plan_trie_score` cuts the tries of a prompt batch into passes of the decoder's layer loop (pure numpy)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np


def _as_ids(x) -> List[int]:
    if hasattr(x, "tolist"):
        x = x.tolist()
    return [int(t) for t in x]


def _encode(tokenizer, text: str) -> List[int]:
    """Ids of `text` without special tokens (a tokenizer without `encode`, as the synthetic presets': its leading BOS dropped)."""
    if hasattr(tokenizer, "encode"):
        return _as_ids(tokenizer.encode(text, add_special_tokens=False))
    ids = _as_ids(tokenizer(text).input_ids)
    bos = getattr(tokenizer, "bos_token_id", None)
    return ids[1:] if ids and bos is not None and ids[0] == bos else ids


class CompiledConstraint:
    """The automaton the device reads.  State 0 is the end state (no edges, completing); state s allows
    edge_tok[edge_off[s] : edge_off[s + 1]] (ascending), moving to edge_next, and the end ids when completing[s]."""

    def __init__(self, edge_off, edge_tok, edge_next, completing, end_ids, start):
        self.edge_off = np.ascontiguousarray(edge_off, dtype=np.int32)
        self.edge_tok = np.ascontiguousarray(edge_tok, dtype=np.int32)
        self.edge_next = np.ascontiguousarray(edge_next, dtype=np.int32)
        self.completing = np.ascontiguousarray(completing, dtype=np.uint8)
        self.end_ids = np.ascontiguousarray(end_ids, dtype=np.int32)
        self.start = np.ascontiguousarray(start, dtype=np.int32)

    @property
    def n_states(self) -> int:
        return len(self.completing)

    @property
    def n_edges(self) -> int:
        return len(self.edge_tok)

    def max_id(self) -> int:
        return int(max(self.end_ids.max(), self.edge_tok.max() if len(self.edge_tok) else -1))

    def min_id(self) -> int:
        return int(min(self.end_ids.min(), self.edge_tok.min() if len(self.edge_tok) else self.end_ids.min()))

    def step(self, state: int, tok: int) -> int:
        """One transition, as the kernel takes it: binary search in the state's ids, 0 when `tok` is no edge."""
        lo, hi = int(self.edge_off[state]), int(self.edge_off[state + 1])
        k = lo + int(np.searchsorted(self.edge_tok[lo:hi], tok))
        return int(self.edge_next[k]) if k < hi and int(self.edge_tok[k]) == tok else 0

    def walk(self, row: int, sent) -> int:
        s = int(self.start[row if len(self.start) > 1 else 0])
        for t in _as_ids(sent):
            s = self.step(s, t)
        return s

    def allowed(self, state: int) -> List[int]:
        ids = self.edge_tok[self.edge_off[state]: self.edge_off[state + 1]].tolist()
        if self.completing[state]:
            ids += self.end_ids.tolist()
        return sorted(set(ids))


class TokenTrie:
    """A closed vocabulary of token sequences (see the module docstring).  sequences: non-empty id lists (duplicates merge);
    end_token_id: an int or a list; separator: the ids between two members of a list answer (None: one member)."""

    def __init__(self, sequences: Sequence[Sequence[int]], end_token_id: Union[int, Sequence[int]],
                 separator: Optional[Sequence[int]] = None):
        if end_token_id is None:
            raise ValueError("TokenTrie needs `end_token_id` (an int or a list of ints)")
        ends = [int(end_token_id)] if isinstance(end_token_id, (int, np.integer)) else _as_ids(end_token_id)
        if not ends:
            raise ValueError("TokenTrie needs at least one end id")
        self.end_ids = sorted(set(ends))
        end_set = set(self.end_ids)
        self.separator = None if separator is None else _as_ids(separator)
        if self.separator is not None and len(self.separator) == 0:
            raise ValueError("`separator` has to be a non-empty list of ids (or None)")
        if self.separator is not None and end_set & set(self.separator):
            raise ValueError(f"an end id inside the separator {self.separator}")
        # the trie: children[n] = {id: node}, complete[n]; node 0 is the root
        self.children: List[dict] = [{}]
        self.complete: List[bool] = [False]
        # for score_trie(): node_tok / node_par / node_depth per node (root: -1, -1, 0); the distinct members in order of first
        # insertion (member_ids, their end nodes member_nodes) and the member index of every sequence passed in (input_member)
        self.node_tok: List[int] = [-1]
        self.node_par: List[int] = [-1]
        self.node_depth: List[int] = [0]
        self.member_ids: List[List[int]] = []
        self.member_nodes: List[int] = []
        self.input_member: List[int] = []
        self.member_strings: Optional[List[str]] = None
        member_of_node: dict = {}
        n_members = 0
        for seq in sequences:
            ids = _as_ids(seq)
            if not ids:
                raise ValueError("an empty member: every sequence of a TokenTrie holds at least one id")
            node = 0
            for t in ids:
                if t in end_set:
                    raise ValueError(f"end id {t} inside the member {ids}")
                if t < 0:
                    raise ValueError(f"negative id {t} in the member {ids}")
                nxt = self.children[node].get(t)
                if nxt is None:
                    nxt = len(self.children)
                    self.children[node][t] = nxt
                    self.children.append({})
                    self.complete.append(False)
                    self.node_tok.append(t)
                    self.node_par.append(node)
                    self.node_depth.append(self.node_depth[node] + 1)
                node = nxt
            self.complete[node] = True
            if node not in member_of_node:
                member_of_node[node] = len(self.member_ids)
                self.member_ids.append(ids)
                self.member_nodes.append(node)
            self.input_member.append(member_of_node[node])
            n_members += 1
        if n_members == 0:
            raise ValueError("TokenTrie needs at least one member")
        if self.separator is not None:
            first = self.separator[0]
            for n, done in enumerate(self.complete):
                if done and first in self.children[n]:
                    raise ValueError(f"ambiguous separator: its first id {first} also continues a member that is complete there")
        self._compiled: Optional[CompiledConstraint] = None
        self._preorder = None
        self._score_plans: dict = {}          # score_trie()'s plans by (prefix rows, include_stop, rows per pass)

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def from_strings(cls, tokenizer, strings: Sequence[str], end_token_id, separator: Optional[str] = None, prefix: str = ""):
        """Members from text: each string is tokenised as `prefix + string` with add_special_tokens=False, the separator likewise
        (without the prefix).  `prefix` exists because most tokenisers encode a word differently behind a space (" nucleus" is
        not "nucleus"): pass the text that precedes the answer in the prompt's continuation, usually " " or ""."""
        members = [_encode(tokenizer, prefix + s) for s in strings]
        sep = None if separator is None else _encode(tokenizer, separator)
        trie = cls(members, end_token_id=end_token_id, separator=sep)
        first = {}
        for s, m in zip(strings, trie.input_member):
            first.setdefault(m, s)
        trie.member_strings = [first[m] for m in range(len(trie.member_ids))]
        return trie

    @staticmethod
    def per_row(tries: Sequence["TokenTrie"]) -> "PerRowTokenTrie":
        """Row b of the batch follows tries[b] (multiple choice: every item its own options)."""
        return PerRowTokenTrie(tries)

    # ------------------------------------------------------------------ the transformers callback
    def allowed_after(self, sent) -> List[int]:
        node, sep_pos = 0, 0                  # sep_pos > 0: inside the separator, that many of its ids seen
        sep = self.separator
        for t in _as_ids(sent):
            if node < 0:
                break
            if sep_pos:
                if t == sep[sep_pos]:
                    sep_pos += 1
                    if sep_pos == len(sep):
                        node, sep_pos = 0, 0
                else:
                    node = -1
                continue
            nxt = self.children[node].get(t)
            if nxt is not None:
                node = nxt
            elif sep is not None and self.complete[node] and t == sep[0]:
                if len(sep) == 1:
                    node = 0
                else:
                    sep_pos = 1
            else:
                node = -1                     # an end id, or an id that was not allowed
        if node < 0:
            return list(self.end_ids)
        if sep_pos:
            return [sep[sep_pos]]
        ids = set(self.children[node])
        if self.complete[node]:
            ids.update(self.end_ids)
            if sep is not None:
                ids.add(sep[0])
        return sorted(ids)

    def __call__(self, batch_id, sent) -> List[int]:
        return self.allowed_after(sent)

    # ------------------------------------------------------------------ the device table
    def _emit(self, base: int):
        """This trie's states numbered from `base` (root first, then breadth-first; the separator's inner states last):
        (edge counts per state, ids, targets, completing) as lists."""
        sep = self.separator
        n_nodes = len(self.children)
        sep_base = base + n_nodes             # state after the separator's first id, second id, ...
        after_first = base if sep is None or len(sep) == 1 else sep_base
        counts, toks, nxts = [], [], []
        for n in range(n_nodes):
            edges = [(t, base + c) for t, c in self.children[n].items()]
            if sep is not None and self.complete[n]:
                edges.append((sep[0], after_first))
            edges.sort()
            counts.append(len(edges))
            toks.extend(e[0] for e in edges)
            nxts.extend(e[1] for e in edges)
        comp = [1 if c else 0 for c in self.complete]
        if sep is not None:
            for k in range(1, len(sep)):      # state sep_base + k - 1: k ids of the separator seen
                counts.append(1)
                toks.append(sep[k])
                nxts.append(base if k + 1 == len(sep) else sep_base + k)
                comp.append(0)
        return counts, toks, nxts, comp

    def compiled(self) -> CompiledConstraint:
        if self._compiled is None:
            self._compiled = _compile([self], [0])
        return self._compiled

    def n_rows(self) -> Optional[int]:
        return None

    # ------------------------------------------------------------------ score_trie()
    @property
    def n_nodes(self) -> int:
        """Nodes below the root."""
        return len(self.children) - 1

    @property
    def max_depth(self) -> int:
        return max(self.node_depth)

    def stop_ids(self) -> List[int]:
        """What a completing state allows besides the children: the end ids, then the separator's first id."""
        return list(self.end_ids) + ([self.separator[0]] if self.separator is not None else [])

    def preorder(self) -> np.ndarray:
        """Nodes >= 1 in depth-first preorder, children in ascending id."""
        if self._preorder is None:
            out, stack = [], [0]
            while stack:
                v = stack.pop()
                if v:
                    out.append(v)
                kids = self.children[v]
                stack.extend(kids[t] for t in sorted(kids, reverse=True))
            self._preorder = np.asarray(out, dtype=np.int32)
        return self._preorder


class PerRowTokenTrie:
    """TokenTrie.per_row: one table, one start state per row.  Every trie has the same end ids."""

    def __init__(self, tries: Sequence[TokenTrie]):
        tries = list(tries)
        if not tries or any(not isinstance(t, TokenTrie) for t in tries):
            raise ValueError("TokenTrie.per_row takes a non-empty list of TokenTrie objects")
        if any(t.end_ids != tries[0].end_ids for t in tries):
            raise ValueError("the tries of TokenTrie.per_row must share their end ids")
        self.tries = tries
        self.end_ids = tries[0].end_ids
        self._compiled: Optional[CompiledConstraint] = None
        self._score_plans: dict = {}

    def __call__(self, batch_id, sent) -> List[int]:
        return self.tries[int(batch_id)].allowed_after(sent)

    def compiled(self) -> CompiledConstraint:
        if self._compiled is None:
            distinct, index, which = [], {}, []
            for t in self.tries:              # a trie shared by several rows is stored once
                if id(t) not in index:
                    index[id(t)] = len(distinct)
                    distinct.append(t)
                which.append(index[id(t)])
            self._compiled = _compile(distinct, which)
        return self._compiled

    def n_rows(self) -> Optional[int]:
        return len(self.tries)

    def row_trie(self, row: int, num_return_sequences: int = 1) -> TokenTrie:
        """The trie decoder row `row` follows.  generate(num_return_sequences=N) runs N rows per prompt, row b N + j being the
        j-th sample of prompt b (transformers' `_expand_inputs_for_generation`): row r follows tries[r // N]."""
        n = int(num_return_sequences)
        if n < 1 or not 0 <= int(row) < len(self.tries) * n:
            raise IndexError(f"row {row} outside the {len(self.tries)} x {n} decoder rows")
        return self.tries[int(row) // n]


def _compile(tries: Sequence[TokenTrie], which: Sequence[int]) -> CompiledConstraint:
    counts, toks, nxts, comp = [0], [], [], [1]           # state 0: the end state
    roots = []
    for t in tries:
        roots.append(len(counts))
        c, k, n, f = t._emit(len(counts))
        counts += c
        toks += k
        nxts += n
        comp += f
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=off[1:])
    if off[-1] >= 2 ** 31 or len(counts) >= 2 ** 31:
        raise ValueError("the constraint's table does not fit 32-bit indices")
    return CompiledConstraint(off, toks, nxts, comp, tries[0].end_ids, [roots[w] for w in which])


# ---------------------------------------------------------------------------------------------------- score_trie(): the plan
TRIE_MAX_DEPTH = 64           # deepest member score_trie() takes (opus_llama_tree_max_depth() of the library says the same)


class TriePass:
    """One pass of the decoder's layer loop.  Per row (arrays of length `rows`): tok, prow (prefix row), parent (row of this pass,
    -1 = the prompt's last position), depth, node, scored (False: an ancestor of the pass's first node, re-computed so that its
    descendants can attend to it, scored in an earlier pass).  score_src: the rows that go through the lm_head - a row of the pass,
    or -(p) - 1 for prefix row p's last position.  Edges (edge_row ascending indices into score_src, edge_tok, edge_slot) and stop
    entries (stop_row ascending, stop_set, stop_slot); slot = p (N + 1) + node."""

    def __init__(self):
        self.tok, self.prow, self.parent, self.depth, self.node, self.scored = [], [], [], [], [], []
        self.score_src, self.edge_row, self.edge_tok, self.edge_slot = [], [], [], []
        self.stop_row, self.stop_set, self.stop_slot = [], [], []

    @property
    def rows(self) -> int:
        return len(self.tok)

    def _freeze(self):
        for k, v in vars(self).items():
            setattr(self, k, np.asarray(v, dtype=bool if k == "scored" else np.int32))
        return self


class TriePlan:
    """plan_trie_score's result: passes; P, N (most nodes below a root), M (most members); tries (the distinct tries) and
    trie_of_row [P]; n_nodes / n_members [P]; rows_evaluated (all passes, re-computed chains included) and evaluated_nodes (without
    them); stop_ids / stop_off (one id set per distinct trie); node_par / node_depth [tries, N + 1] and member_node [tries, M]
    (-1 beyond a trie's own count) for the path sums."""


def plan_trie_score(tries: Sequence[TokenTrie], include_stop: bool, rows_cap: int) -> TriePlan:
    """The passes that score tries[p] behind prefix row p (the same object for rows that share a trie).

    Evaluated nodes: without a stop term the nodes >= 1 that have a child (a leaf's token is scored from its parent's logits and
    nobody attends to a leaf), with it every node >= 1.  Order: prefix row by prefix row, each trie in preorder (children in
    ascending id).  A pass is a run of that order of at most rows_cap rows, the ancestors of its first node included: in preorder
    every other parent lies inside the run.  Passes may mix prefix rows.  A root's edges (scored from the prompt's last position)
    go with the pass that begins its prefix row and cost no row."""
    tries = list(tries)
    if not tries or any(not isinstance(t, TokenTrie) for t in tries):
        raise TypeError("plan_trie_score takes a non-empty list of TokenTrie objects")
    deepest = max(t.max_depth for t in tries)
    if deepest > TRIE_MAX_DEPTH:
        raise ValueError(f"a member of {deepest} ids: score_trie() takes tries up to depth {TRIE_MAX_DEPTH}")
    if rows_cap < deepest:
        raise ValueError(f"rows_cap={rows_cap} cannot hold a chain of depth {deepest}")
    plan = TriePlan()
    distinct, index = [], {}
    for t in tries:
        if id(t) not in index:
            index[id(t)] = len(distinct)
            distinct.append(t)
    P, N, M = len(tries), max(t.n_nodes for t in tries), max(len(t.member_ids) for t in tries)
    plan.P, plan.N, plan.M, plan.include_stop = P, N, M, bool(include_stop)
    plan.tries = distinct
    plan.trie_of_row = np.asarray([index[id(t)] for t in tries], dtype=np.int32)
    plan.n_nodes = np.asarray([t.n_nodes for t in tries], dtype=np.int64)
    plan.n_members = np.asarray([len(t.member_ids) for t in tries], dtype=np.int64)
    plan.node_par = np.full((len(distinct), N + 1), -1, dtype=np.int32)
    plan.node_depth = np.zeros((len(distinct), N + 1), dtype=np.int32)
    plan.member_node = np.full((len(distinct), M), -1, dtype=np.int32)
    off, ids = [0], []
    for k, t in enumerate(distinct):
        plan.node_par[k, : t.n_nodes + 1] = t.node_par
        plan.node_depth[k, : t.n_nodes + 1] = t.node_depth
        plan.member_node[k, : len(t.member_nodes)] = t.member_nodes
        ids += t.stop_ids()
        off.append(len(ids))
    plan.stop_ids = np.asarray(ids, dtype=np.int32)
    plan.stop_off = np.asarray(off, dtype=np.int32)

    passes, cur, row_of = [], TriePass(), {}
    evaluated = 0

    def close():
        nonlocal cur, row_of
        if cur.rows or len(cur.score_src):
            passes.append(cur._freeze())
        cur, row_of = TriePass(), {}

    def add_row(t, p, v, scored):
        row_of[v] = cur.rows
        cur.tok.append(t.node_tok[v])
        cur.prow.append(p)
        cur.parent.append(-1 if t.node_par[v] == 0 else row_of[t.node_par[v]])
        cur.depth.append(t.node_depth[v])
        cur.node.append(v)
        cur.scored.append(scored)

    def add_edges(t, p, v, src):
        """Node v's logits (source `src`) score its children and, in a completing state with a stop term, the stop ids."""
        kids = t.children[v]
        stop = include_stop and t.complete[v]
        if not kids and not stop:
            return
        k = len(cur.score_src)
        cur.score_src.append(src)
        for tok in sorted(kids):
            cur.edge_row.append(k)
            cur.edge_tok.append(tok)
            cur.edge_slot.append(p * (N + 1) + kids[tok])
        if stop:
            cur.stop_row.append(k)
            cur.stop_set.append(index[id(t)])
            cur.stop_slot.append(p * (N + 1) + v)

    for p, t in enumerate(tries):
        row_of = {}                                            # (rows of another prefix row are no parents of this one's)
        add_edges(t, p, 0, -p - 1)
        for v in t.preorder().tolist():
            if not include_stop and not t.children[v]:
                continue
            if cur.rows >= rows_cap:
                close()
            if t.node_par[v] != 0 and t.node_par[v] not in row_of:      # a fresh pass in the middle of a trie: the chain first
                chain, a = [], t.node_par[v]
                while a != 0:
                    chain.append(a)
                    a = t.node_par[a]
                for a in reversed(chain):
                    add_row(t, p, a, False)
            add_row(t, p, v, True)
            add_edges(t, p, v, cur.rows - 1)
            evaluated += 1
    close()
    plan.passes = passes
    plan.evaluated_nodes = evaluated
    plan.rows_evaluated = int(sum(ps.rows for ps in passes))
    return plan


# ---------------------------------------------------------------------------------------------------- search_trie(): the table
TRIE_SEARCH_MAX_BEAMS = 16    # beams per prompt search_trie() takes (the expand kernel's register lists)


class TrieSearchTable:
    """What search_trie() uploads (opus_set_trie_search): the children of the distinct tries in CSR form.  State 0 is the dead state;
    node n of distinct trie k is state root[k] + n, so a state minus its root is score_trie()'s node number.  edge_off / edge_tok
    (ascending within a state) / edge_next; member [states]: the member index of a node that completes a member, -1 otherwise;
    stop_set [states]: the trie's entry in stop_off / stop_ids (TokenTrie.stop_ids(): what score_trie's stop term sums);
    start [P]: the root of prompt p's trie.  The separator's edges are not part of it: the search ends at one member."""

    def __init__(self, tries: Sequence[TokenTrie]):
        tries = list(tries)
        if not tries or any(not isinstance(t, TokenTrie) for t in tries):
            raise TypeError("TrieSearchTable takes a non-empty list of TokenTrie objects")
        distinct, index = [], {}
        for t in tries:
            if id(t) not in index:
                index[id(t)] = len(distinct)
                distinct.append(t)
        counts, toks, nxts, member, sset, roots, soff, sids = [0], [], [], [-1], [0], [], [0], []
        for k, t in enumerate(distinct):
            base = len(counts)
            roots.append(base)
            of_node = {n: m for m, n in enumerate(t.member_nodes)}
            for n, kids in enumerate(t.children):
                counts.append(len(kids))
                for tok in sorted(kids):
                    toks.append(tok)
                    nxts.append(base + kids[tok])
                member.append(of_node.get(n, -1))
                sset.append(k)
            sids += t.stop_ids()
            soff.append(len(sids))
        off = np.zeros(len(counts) + 1, dtype=np.int64)
        np.cumsum(np.asarray(counts, dtype=np.int64), out=off[1:])
        if off[-1] >= 2 ** 27 or len(counts) >= 2 ** 31:
            raise ValueError("the trie's table does not fit the search kernel's 27-bit edge numbers")
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                           # noqa: E731
        self.tries = distinct
        self.edge_off, self.edge_tok, self.edge_next = i32(off), i32(toks), i32(nxts)
        self.member, self.stop_set, self.stop_off, self.stop_ids = i32(member), i32(sset), i32(soff), i32(sids)
        self.root = i32(roots)
        self.trie_of_row = i32([index[id(t)] for t in tries])
        self.start = self.root[self.trie_of_row]
        self.max_depth = max(t.max_depth for t in distinct)

    @property
    def n_states(self) -> int:
        return len(self.member)

    @property
    def n_edges(self) -> int:
        return len(self.edge_tok)


def is_constraint(obj) -> bool:
    return isinstance(obj, (TokenTrie, PerRowTokenTrie))
