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
banned by another processor (min_new_tokens larger than its shortest member, a bad word) is the caller's error."""
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
                node = nxt
            self.complete[node] = True
            n_members += 1
        if n_members == 0:
            raise ValueError("TokenTrie needs at least one member")
        if self.separator is not None:
            first = self.separator[0]
            for n, done in enumerate(self.complete):
                if done and first in self.children[n]:
                    raise ValueError(f"ambiguous separator: its first id {first} also continues a member that is complete there")
        self._compiled: Optional[CompiledConstraint] = None

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def from_strings(cls, tokenizer, strings: Sequence[str], end_token_id, separator: Optional[str] = None, prefix: str = ""):
        """Members from text: each string is tokenised as `prefix + string` with add_special_tokens=False, the separator likewise
        (without the prefix).  `prefix` exists because most tokenisers encode a word differently behind a space (" nucleus" is
        not "nucleus"): pass the text that precedes the answer in the prompt's continuation, usually " " or ""."""
        members = [_encode(tokenizer, prefix + s) for s in strings]
        sep = None if separator is None else _encode(tokenizer, separator)
        return cls(members, end_token_id=end_token_id, separator=sep)

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


def is_constraint(obj) -> bool:
    return isinstance(obj, (TokenTrie, PerRowTokenTrie))
