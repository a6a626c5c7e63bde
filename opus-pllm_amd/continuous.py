"""Schedule of generate_continuous(): which prompt takes which decode row at which step (host side, no device call).

A *session* is one live decode batch of B <= slots rows.  Its step t writes every row's token to cache slot T0 + t and to column t
of the id buffer [B, S]; S is the session's step budget.  A row's occupant that began at step `start` is done at the first step
`end` at which it emitted an EOS id, completed the stop sequence or has emitted max_new tokens (end - start + 1 of them).

    1. a session opens with the ordinary prefill of the next min(slots, queued) prompts, left-padded to their longest T0;
    2. at a step boundary t a free row takes the next queued prompt with  len <= T0 + t  and  t + max_new <= S; prompts that do
       not fit yet stay queued and later ones may overtake them;
    3. the session ends when every row is done and nothing can be refilled, or at t == S;
    4. at boundary t the host knows the rows' state as of step t - LAG only, so the schedule is a function of the prompts'
       lengths and the answers' lengths - never of how far the device happens to be.

run_schedule() drives a backend (the device one of model.py, or SimBackend here, which replays recorded answer lengths); both see
the same decisions, which is what makes the schedule testable on the CPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

LAG = 3          # steps between what the host enqueues and what it has seen (opus_stream_lag(): the poll ring's lag + 1)

STAT_KEYS = ("sessions", "decode_steps", "refills", "rows_refilled", "live_row_steps", "slot_steps")


def default_refill_min(slots: int) -> int:
    return max(1, int(slots) // 4)


def pick_refill(queue: Sequence[int], lens: Sequence[int], free_rows: Sequence[int], t: int, T0: int, max_new: int,
                S: int) -> List[Tuple[int, int]]:
    """Rule 2: [(row, prompt)] - the free rows in ascending order take the queued prompts that fit, in queue order."""
    if t + max_new > S:
        return []
    fit = [p for p in queue if lens[p] <= T0 + t]
    return list(zip(sorted(free_rows), fit))


def run_args(queue: Sequence[int], lens: Sequence[int], t: int, T0: int, max_new: int, S: int, B: int,
             refill_min: int) -> Tuple[int, int]:
    """(t_min, min_free) of the next run from boundary t: the run stops at the first boundary t' >= t_min at which min_free rows
    are known to be done (and always when all B are, or at S).  With nothing left to refill - an empty queue, or no boundary
    left at which a new row could still end inside S - min_free is out of reach (B + 1): the session drains.  t_min is the first
    boundary at which the shortest queued prompt fits under the session's slots, so a run never returns for nothing."""
    t_min = t + 1
    if queue:
        t_min = max(t_min, min(lens[p] for p in queue) - T0)
    if not queue or t_min + max_new > S:
        return t + 1, B + 1
    return t_min, max(1, min(int(refill_min), B))


def stream_stop(t: int, t_min: int, min_free: int, t_max: int, start: Sequence[int], end: Sequence[int],
                lag: int = LAG) -> Tuple[int, List[int]]:
    """What opus_stream_run returns from boundary t when row r's occupant began at start[r] and is done at step end[r] (-1: not
    inside this session): (t', the end steps known at t', -1 elsewhere).  A pure mirror of the native loop."""
    B = len(start)
    while True:
        sv = t - lag
        seen = [end[r] if (0 <= end[r] <= sv and start[r] <= sv) else -1 for r in range(B)]
        ndone = sum(1 for e in seen if e >= 0)
        if ndone == B or t >= t_max or (t >= t_min and ndone >= min_free):
            return t, seen
        t += 1


class SimBackend:
    """Replays recorded answer lengths: prompt p emits n_tokens[p] ids (<= max_new) wherever it runs."""

    def __init__(self, n_tokens: Sequence[int], lag: int = LAG):
        self.n_tokens, self.lag = [int(n) for n in n_tokens], lag
        self.log: List[tuple] = []           # ("begin", prompts, T0) / ("refill", t, [(row, prompt)]) / ("end", t)
        self.harvested: List[Tuple[int, int, int, int]] = []

    def begin(self, prompts, T0):
        self.start = [0] * len(prompts)
        self.end = [self.n_tokens[p] - 1 for p in prompts]
        self.t = 0
        self.log.append(("begin", tuple(prompts), T0))

    def run(self, t_min, min_free, t_max):
        self.t, seen = stream_stop(self.t, t_min, min_free, t_max, self.start, self.end, self.lag)
        return self.t, seen

    def harvest(self, prompt, row, start, end):
        self.harvested.append((prompt, row, start, end))

    def refill(self, assign, t, L):
        for r, p in assign:
            self.start[r], self.end[r] = t, t + self.n_tokens[p] - 1
        self.log.append(("refill", t, tuple(assign)))

    def finish(self):
        self.log.append(("end", self.t))
        return [e if e < self.t else -1 for e in self.end]


def check_capacity(lens: Sequence[int], slots: int, max_new: int, S: int, max_prompt: int, max_batch: int) -> Optional[str]:
    """The capacity violation of a call, or None."""
    if slots < 1 or slots > max_batch:
        return f"slots={slots}: the context holds max_batch={max_batch} decode rows"
    if max_new < 1 or max_new > S:
        return f"max_new_tokens={max_new} exceeds the session's step budget, the context's max_new_tokens={S}"
    for p, n in enumerate(lens):
        if n < 1 or n > max_prompt:
            return f"prompt {p} takes {n} positions after the splice: the context holds max_prompt={max_prompt}"
    return None


def run_schedule(lens: Sequence[int], slots: int, max_new: int, S: int, refill_min: Optional[int], backend) -> dict:
    """Runs every prompt (spliced lengths `lens`, queued in input order) through `backend` and returns the statistics
    (STAT_KEYS) plus "placements": per prompt (session, row, start step).  sessions: decode batches opened; decode_steps: steps
    enqueued; refills: refill launches; rows_refilled: rows a prompt took after the call's first prefill (by a refill, or by a
    later session's opening prefill) = N - the first batch; live_row_steps: steps at which a row emitted an id that is returned
    (= the sum of the answers' lengths); slot_steps: rows x steps of every session.  Every loop is bounded: a run advances t
    (<= S), a refill shortens the queue, a session takes at least one prompt."""
    N = len(lens)
    refill_min = default_refill_min(slots) if refill_min is None else int(refill_min)
    if refill_min < 1:
        raise ValueError("`refill_min` has to be at least 1")
    queue = list(range(N))
    stats = {k: 0 for k in STAT_KEYS}
    placements: List[Optional[Tuple[int, int, int]]] = [None] * N
    while queue:
        first = queue[:slots]
        del queue[:len(first)]
        B, T0 = len(first), max(lens[p] for p in first)
        session = stats["sessions"]
        stats["sessions"] += 1
        if session:                          # rows_refilled: every row a prompt took after the call's first prefill
            stats["rows_refilled"] += B
        backend.begin(first, T0)
        occ: List[Optional[int]] = list(first)
        start = [0] * B
        for r, p in enumerate(first):
            placements[p] = (session, r, 0)
        t = 0

        def harvest(r, e):
            backend.harvest(occ[r], r, start[r], e)
            stats["live_row_steps"] += e - start[r] + 1
            occ[r] = None

        while True:
            t_min, min_free = run_args(queue, lens, t, T0, max_new, S, B, refill_min)
            t, end = backend.run(t_min, min_free, S)
            for r in range(B):
                if occ[r] is not None and end[r] >= 0:
                    harvest(r, end[r])
            free = [r for r in range(B) if occ[r] is None]
            assign = pick_refill(queue, lens, free, t, T0, max_new, S)
            if assign:
                backend.refill(assign, t, T0 + t)
                for r, p in assign:
                    queue.remove(p)
                    occ[r], start[r] = p, t
                    placements[p] = (session, r, t)
                stats["refills"] += 1
                stats["rows_refilled"] += len(assign)
                continue
            if len(free) == B or t >= S:
                break
        final = backend.finish()
        for r in range(B):
            if occ[r] is not None:
                if final[r] < 0:
                    raise RuntimeError(f"row {r} of session {session} was still owed tokens at step {t}")
                harvest(r, final[r])
        stats["decode_steps"] += t
        stats["slot_steps"] += B * t
    stats["placements"] = placements
    return stats


def simulate(lens: Sequence[int], n_tokens: Sequence[int], slots: int, max_new: int, S: int, refill_min: Optional[int] = None,
             lag: int = LAG):
    """The schedule of a call whose prompt p answers with n_tokens[p] ids: (statistics, SimBackend with its log)."""
    sim = SimBackend(n_tokens, lag)
    return run_schedule(lens, slots, max_new, S, refill_min, sim), sim
