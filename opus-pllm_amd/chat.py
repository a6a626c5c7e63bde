"""Multi-turn conversations on one decoder context: every turn keeps the KV cache of its prompt AND of the answer it generated, so
the next turn prefills only what the user adds.

    chat = opa.ChatSession(model)                 # B independent conversations in lockstep (row b of every call is conversation b)
    a1 = chat.ask(ids1, seq=proteins, attention_mask=m1, max_new_tokens=64, eos_token_id=eos)
    a2 = chat.ask(ids2, attention_mask=m2, max_new_tokens=64, eos_token_id=eos)
    chat.rewind(1)                                # forget the last turn; the next ask() continues behind the first answer

The first ask() is generate(..., return_dict_in_generate=True, return_prefix=True); every later one is the same call with
prefix=chat.prefix.  A turn's handle is a detached OpusPrefix: an immutable copy of the rows' K / V, right-aligned, the last
generated id of every row `pending` (model.generate's docstring).  The conversation the engine sees is the concatenation of the ID
segments - first prompt, answer ids up to and including each row's EOS / stop id, next ids, ... - not a re-tokenisation of the
rendered text; conversation.Conversation.turn_delta() renders the text a follow-up adds.

What a handle costs: prefix.snapshot_bytes(layers, kv_heads, head_dim, rows, slots) bytes of device memory (OpusPrefix.nbytes()),
131 072 bytes per slot and row at the Llama-3-8B shape, for `slots` = the longest conversation of the batch.  The session keeps the
latest handle and the one before it (one rewind); keep_handles=True keeps every turn's.  The conversation has to fit the context's
max_prompt (slots + the follow-up's width <= max_prompt), else OpusError -2 names the max_prompt that would have sufficed.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch


class ChatSession:
    """B conversations in lockstep on `model`'s context.  `prefix`: the latest handle (None before the first turn); `lengths`
    [B]: cache slots every row uses; `turns`: [(ids_in, ids_out), ...] as given and as generated (CPU tensors)."""

    def __init__(self, model, keep_handles: bool = False):
        self.model = model
        self.keep_handles = bool(keep_handles)
        self.turns: List[Tuple[torch.Tensor, torch.Tensor]] = []
        self._handles: List[Optional[object]] = []          # handle behind turn i (None once dropped)

    @property
    def prefix(self):
        return self._handles[-1] if self._handles else None

    @property
    def lengths(self) -> Optional[torch.Tensor]:
        return None if self.prefix is None else self.prefix.lengths

    def ask(self, input_ids: torch.Tensor, seq=None, **kwargs):
        """One turn: generate() on the first turn's prompt, generate(prefix=self.prefix) on a follow-up's ids.  Every other
        generate() argument is forwarded; returns what generate() returns (return_dict_in_generate defaults to True, and a call
        that passes False gets the new ids as plain generate() would)."""
        if "prefix" in kwargs or "return_prefix" in kwargs:
            raise ValueError("ChatSession.ask() sets prefix / return_prefix itself")
        as_dict = bool(kwargs.pop("return_dict_in_generate", True))
        if self.prefix is not None:
            kwargs["prefix"] = self.prefix
        out = self.model.generate(input_ids, seq, return_dict_in_generate=True, return_prefix=True, **kwargs)
        self._handles.append(out.prefix)
        if not self.keep_handles:
            for i in range(len(self._handles) - 2):          # the latest and the one before it stay
                self._handles[i] = None
        self.turns.append((input_ids.detach().cpu(), out.sequences.detach().cpu()))
        return out if as_dict else out.sequences

    def rewind(self, n: int = 1) -> None:
        """Forgets the last n turns: the next ask() continues behind the turn before them (n = all of them: a new conversation).
        Handles are immutable copies, so nothing is recomputed; ValueError when the handle to go back to was not kept
        (keep_handles=False keeps one step)."""
        n = int(n)
        if n < 0 or n > len(self.turns):
            raise ValueError(f"rewind({n}) on a session of {len(self.turns)} turns")
        left = len(self.turns) - n
        if n and left and self._handles[left - 1] is None:
            raise ValueError(f"the handle behind turn {left} was dropped: create the session with keep_handles=True")
        del self.turns[left:], self._handles[left:]

    def reset(self) -> None:
        self.rewind(len(self.turns))
