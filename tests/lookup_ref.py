"""CPU twin of prompt-lookup decoding (csrc/lookup.hip, opus_generate_lookup): the draft rule, acceptance and commit in lockstep,
and the whole loop over a `step_fn` that plays the model.  Plain Python on lists of ints; every rule is restated here, not
imported from the package, so that the kernels and the host loop are checked against an independent statement.

History of a row: prompt ids without padding, -1 where a protein block was spliced in, then optionally -1 and a corpus, then the
ids generated so far."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

SENTINEL = -1


def draft(h: Sequence[int], k: int, max_ngram: int = 2) -> List[int]:
    """Transformers' PromptLookupCandidateGenerator.get_candidates rule on one history, with the sentinel rules: for m from
    min(max_ngram, len - 1) down to 1 the first window start i (left to right) with h[i:i+m] == h[len-m:], a continuation
    (i + m < len) that does not begin with -1; the draft is h[i+m : min(i+m+k, len)], cut in front of a -1.  A window that
    contains -1 never matches."""
    n = len(h)
    for m in range(min(max_ngram, n - 1), 0, -1):
        tail = list(h[n - m:])
        if SENTINEL in tail:
            continue
        for i in range(0, n - m):
            if list(h[i:i + m]) == tail and h[i + m] != SENTINEL:
                out = []
                for t in h[i + m:min(i + m + k, n)]:
                    if t == SENTINEL:
                        break
                    out.append(int(t))
                return out
    return []


def history(prompt_ids: Sequence[int], mask: Optional[Sequence[int]] = None, corpus: Optional[Sequence[int]] = None,
            placeholder: int = -200, n_prot_tokens: int = 1) -> List[int]:
    """The searchable history of one prompt row: its unpadded ids, n_prot_tokens sentinels for a <seq> placeholder, and behind one
    more sentinel the caller's corpus."""
    h: List[int] = []
    for j, t in enumerate(prompt_ids):
        if mask is not None and not mask[j]:
            continue
        h.extend([SENTINEL] * n_prot_tokens if int(t) == placeholder else [int(t)])
    if corpus is not None and len(corpus):
        h.append(SENTINEL)
        h.extend(int(t) for t in corpus)
    return h


def accept_len(x: Sequence[int], y: Sequence[int], draft_len: int) -> int:
    """m_b: the longest j <= draft_len with x[i] == y[i-1] for all 1 <= i <= j."""
    m = 0
    while m < min(draft_len, len(x) - 1) and x[m + 1] == y[m]:
        m += 1
    return m


class State:
    """The decode loop's bookkeeping: the id matrix [R][stride] (pad-filled), the finished flags, the step word (cache slots
    behind the prompt), the last committed id per row, the rows unfinished behind every column."""

    def __init__(self, R: int, stride: int, pad: int):
        self.ids = [[pad] * stride for _ in range(R)]
        self.fin = [0] * R
        self.step = 0
        self.next = [pad] * R
        self.n_unf = [0] * stride
        self.pad = pad
        self.stride = stride

    def n_out(self) -> int:
        """Columns produced (transformers stops once every row has finished), given step + 1 columns were committed."""
        produced = self.step + 1
        for q in range(produced):
            if self.n_unf[q] == 0:
                return q + 1
        return produced


def commit(st: State, x: List[List[int]], y: List[List[int]], draft_len: Sequence[int], pre: int, eos: Sequence[int] = (),
           stop: Sequence[int] = ()) -> Tuple[int, int, int]:
    """Lockstep acceptance and commit of one pass (pre = 1) or of the ids behind a plain step / the prefill (pre = 0, one position).
    Returns (a, rows unfinished, ids drafted by unfinished rows)."""
    R, n = len(y), len(y[0])
    base = st.step + pre
    ms, drafted = [], 0
    for b in range(R):
        if st.fin[b]:
            continue
        dl = max(0, min(draft_len[b], n - 1))
        drafted += dl
        ms.append(accept_len(x[b][:n], y[b], dl))
    a = min(ms) if ms else 0
    a = min(a, st.stride - 1 - base)
    if a >= 0:
        for b in range(R):
            f, tok = st.fin[b], st.pad
            for j in range(a + 1):
                col = base + j
                tok = st.pad if f else y[b][j]
                st.ids[b][col] = tok
                if not f and tok in eos:
                    f = 1
                if not f and stop and col + 1 >= len(stop) and st.ids[b][col - len(stop) + 1:col + 1] == list(stop):
                    f = 1
                if not f:
                    st.n_unf[col] += 1
            st.fin[b] = f
            st.next[b] = tok
        st.step += pre * (a + 1)
    return max(a, 0), sum(1 for f in st.fin if not f), drafted


def commit_per_row(st: State, x, y, draft_len, pre, eos=(), stop=()):
    """The same outcome stated row by row (the check of `commit`): each row walks its own chain to its own m_b, and only then is
    every row cut back to the shortest chain of a row that was unfinished at the start."""
    R, n = len(y), len(y[0])
    base = st.step + pre
    chains = []
    for b in range(R):
        if st.fin[b]:
            chains.append(None)
            continue
        dl = max(0, min(draft_len[b], n - 1))
        j = 0
        while j < dl and x[b][j + 1] == y[b][j]:
            j += 1
        chains.append(j)
    live = [c for c in chains if c is not None]
    a = min(min(live) if live else 0, st.stride - 1 - base)
    for b in range(R):
        row = st.ids[b]
        done = bool(st.fin[b])
        last = st.pad
        for col in range(base, base + a + 1):
            last = st.pad if done else y[b][col - base]
            row[col] = last
            if done:
                continue
            if last in eos or (stop and col + 1 >= len(stop) and row[col + 1 - len(stop):col + 1] == list(stop)):
                done = True
            else:
                st.n_unf[col] += 1
        if a >= 0:
            st.fin[b] = int(done)
            st.next[b] = last
    if a >= 0:
        st.step += pre * (a + 1)
    return max(a, 0), sum(1 for f in st.fin if not f), sum(max(0, min(draft_len[b], n - 1)) for b in range(R) if chains[b] is not None)


def generate(step_fn: Callable[[int, List[int]], int], hists: List[List[int]], max_new: int, k: int, max_ngram: int = 2,
             eos: Sequence[int] = (), stop: Sequence[int] = (), pad: int = 0):
    """The whole loop.  step_fn(b, generated ids of row b) -> the model's greedy next id for row b behind those ids (a pure
    function: the twin of exact verification).  Returns (ids [R][n_out], stats dict)."""
    R = len(hists)
    st = State(R, max_new, pad)
    stats = {"passes": 0, "plain_steps": 0, "drafted": 0, "accepted": 0}

    def fed(b, upto):            # ids of row b the model has seen behind the prompt, finished rows included (pads)
        return st.ids[b][:upto]

    y = [[step_fn(b, [])] for b in range(R)]
    _, unf, _ = commit(st, [[pad]] * R, y, [0] * R, 0, eos, stop)
    while st.step + 1 < max_new and unf > 0:
        C = st.step + 1
        drafts = [[] if st.fin[b] else draft(hists[b] + st.ids[b][:C], k, max_ngram) for b in range(R)]
        n = min(1 + max(len(d) for d in drafts), max_new - C)
        if n <= 1:
            y = [[step_fn(b, fed(b, C))] for b in range(R)]
            st.step += 1                                           # (the plain step advances the word itself)
            _, unf, _ = commit(st, [[st.next[b]] for b in range(R)], y, [0] * R, 0, eos, stop)
            stats["plain_steps"] += 1
            continue
        x = [[st.next[b]] + (drafts[b] + [pad] * n)[:n - 1] for b in range(R)]
        y = [[step_fn(b, fed(b, C - 1) + x[b][:j + 1]) for j in range(n)] for b in range(R)]
        a, unf, dr = commit(st, x, y, [len(d) for d in drafts], 1, eos, stop)
        stats["passes"] += 1
        stats["drafted"] += dr
        stats["accepted"] += a
    n_out = st.n_out()
    return [row[:n_out] for row in st.ids], stats


def generate_plain(step_fn, R: int, max_new: int, eos=(), stop=(), pad: int = 0):
    """Plain greedy search with the same bookkeeping (what the lookup loop has to equal id for id)."""
    ids = [[pad] * max_new for _ in range(R)]
    fin = [False] * R
    n_out = max_new
    for col in range(max_new):
        for b in range(R):
            tok = pad if fin[b] else step_fn(b, ids[b][:col])
            ids[b][col] = tok
            if not fin[b] and (tok in eos or (stop and col + 1 >= len(stop) and ids[b][col + 1 - len(stop):col + 1] == list(stop))):
                fin[b] = True
        if all(fin):
            n_out = col + 1
            break
    return [row[:n_out] for row in ids]
