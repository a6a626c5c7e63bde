"""Prompt assembly of the batch annotation driver (eval/run_opus_ddp.py:90-108).

Only what that driver reads from the reference's conversation presets is kept here: the v0 system text, the two
role names and the separator (multi_modality_v1/conversation.py:159-167); the full conversation class lives in
`conversation.py`.  Also the host-side pieces of the other two eval scripts: the multiple-choice
question template and answer scoring (eval_run_multichoice.py:76-83,171-206) and the interactive script's input check
and prompt (run_opus_online.py:12-14,40-58).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

from .constants import DEFAULT_SEQ_TOKEN


@dataclass(frozen=True)
class PromptPreset:
    system: str
    roles: Tuple[str, str]
    sep: str


conv_vicuna_v0 = PromptPreset(
    system="A chat between a curious student and a biological professor who is familiar with protein properties. "
           "The biological professor gives helpful, detailed, and professional answers to student's questions.",
    roles=("Student", "Professor"), sep="###")


def max_new_tokens_for(input_path: str) -> int:
    """Generation budget chosen by substring of the dataset path (run_opus_ddp.py:93-101)."""
    if "localization" in input_path:
        return 32
    if "keywords" in input_path:
        return 128
    return 256


def build_prompt(instruction: str, input_path: str = "", conv: PromptPreset = conv_vicuna_v0) -> str:
    """header + '### Student: <seq>\\n{instruction}\\n### Professor:' (run_opus_ddp.py:90-108)."""
    if DEFAULT_SEQ_TOKEN not in instruction:
        if "localization" in input_path:
            instruction = DEFAULT_SEQ_TOKEN + "\n" + instruction + "Kindly reply with only one word."
        else:
            instruction = DEFAULT_SEQ_TOKEN + "\n" + instruction
    return f"{conv.system}\n\n### {conv.roles[0]}: {instruction}\n### Professor:"


def after_process_output(outputs: str, conv: PromptPreset = conv_vicuna_v0) -> str:
    """Cut the decoded text at the first separator (run_opus_ddp.py:19-27)."""
    outputs = outputs.strip()
    idx = outputs.find(conv.sep)
    return (outputs if idx < 0 else outputs[:idx]).strip()


# ------------------------------------------------------------------------------------------------ multiple choice
import re as _re

_OPTION = _re.compile(r"\b([A-Da-d])[\s]*[).\.）\]】]|answer\s*:\s*([A-Da-d])|答案是\s*([A-Da-d])", _re.IGNORECASE)


def multichoice_prompt(question: str, options) -> str:
    """Question text of eval_run_multichoice.py:76-83 (options joined by newlines, :93-94); the indentation of the
    reference's triple-quoted literal is part of the prompt."""
    opts = options if isinstance(options, str) else "\n".join(options)
    return (f"Question: {question}\n\n        Options:\n        {opts}\n\n"
            "        Please carefully read the question and select the single correct answer from A-D.\n"
            "        You can only output one option from A), B), C), D) with format 'The correct answer is' without explanation.")


def extract_option_letter(text: str):
    """First `A)` / `b.` / `answer: c` / `答案是 D` style option in `text`, upper-cased; the text itself when there is
    none (eval_run_multichoice.py:176-187)."""
    m = _OPTION.search(text)
    if not m:
        return text
    letter = next((g for g in m.groups() if g is not None), None)
    return letter.upper() if letter else None


def score_multichoice(records):
    """records: [{'ground_truth', 'generated'}] -> (n_correct, per-option histogram) (eval_run_multichoice.py:189-210)."""
    hist = {"A": 0, "B": 0, "C": 0, "D": 0, "None": 0}
    correct = 0
    for r in records:
        got, want = extract_option_letter(r["generated"]), extract_option_letter(r["ground_truth"])
        correct += int(got == want)
        if got is not None and got in hist:
            hist[got] += 1
        else:
            hist["None"] += 1
    return correct, hist


# ------------------------------------------------------------------------------------------------ interactive script
_AMINO = frozenset("ACDEFGHIKLMNPQRSTVWY")


def is_protein_sequence(seq: str) -> bool:
    """Only the 20 standard residues, case-insensitive; the empty string passes (run_opus_online.py:12-14)."""
    return all(ch in _AMINO for ch in seq.upper())


def online_prompt(instruction: str, has_sequence: bool, conv=conv_vicuna_v0):
    """(prompt, instruction as shown) of run_opus_online.py:40-58: the <seq> placeholder is prepended only when a
    sequence is given and the instruction does not already carry it; the answer cue is always 'Professor:'."""
    if has_sequence and DEFAULT_SEQ_TOKEN not in instruction:
        instruction = DEFAULT_SEQ_TOKEN + "\n" + instruction
    return f"{conv.system}\n\n### {conv.roles[0]}: {instruction}\n### Professor:", instruction


def online_followup(instruction: str, has_sequence: bool, conv=conv_vicuna_v0, after_separator: bool = False):
    """(text, instruction as shown) a follow-up turn of eval_online.py --multi_turn adds behind the previous answer, in
    online_prompt's own format: the separator line that closes the answer (left out when the answer already ended with the
    separator: after_separator), the student's turn, the answer cue."""
    if has_sequence and DEFAULT_SEQ_TOKEN not in instruction:
        instruction = DEFAULT_SEQ_TOKEN + "\n" + instruction
    head = " " if after_separator else "\n### "
    return f"{head}{conv.roles[0]}: {instruction}\n### Professor:", instruction


def online_cut(outputs: str, sep: str = "###") -> str:
    """Text up to the first separator found from offset 2 (run_opus_online.py:86-92)."""
    outputs = outputs.strip()
    idx = outputs.find(sep, 2)
    return (outputs if idx < 0 else outputs[:idx]).strip()


def add_logits_processor_args(p) -> None:
    """The drivers' generate() logits processors (transformers' options; all off by default, as in the reference's drivers)."""
    p.add_argument("--repetition_penalty", type=float, default=None,
                   help="penalise every id the row has generated (s / p, or s * p for s < 0); 1.0 / unset: off")
    p.add_argument("--no_repeat_ngram_size", type=int, default=None,
                   help="never repeat an n-gram of the generated ids; 0 / unset: off")
    p.add_argument("--min_new_tokens", type=int, default=None,
                   help="EOS is banned until this many ids have been generated; unset: off")


def add_warper_args(p) -> None:
    """The drivers' truncation warpers of generate(do_sample=True) (transformers' options, behind top-k / top-p; all off by default)."""
    p.add_argument("--min_p", type=float, default=None, help="keep tokens with at least min_p times the top token's probability")
    p.add_argument("--typical_p", type=float, default=None, help="locally typical sampling: the mass kept around the entropy; 1.0 / unset: off")
    p.add_argument("--epsilon_cutoff", type=float, default=None, help="drop tokens whose probability is below this; 0 / unset: off")
    p.add_argument("--eta_cutoff", type=float, default=None, help="the same with min(eta, sqrt(eta) exp(-entropy)); 0 / unset: off")


def warper_kwargs(args) -> dict:
    """generate() keywords of add_warper_args' options (unset ones are left out)."""
    names = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
    return {k: getattr(args, k) for k in names if getattr(args, k, None) is not None}


def logits_processor_kwargs(args) -> dict:
    """generate() keywords of add_logits_processor_args' options (unset ones are left out)."""
    names = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens")
    return {k: getattr(args, k) for k in names if getattr(args, k, None) is not None}


def add_lookup_args(p) -> None:
    """The drivers' prompt-lookup decoding (generate(prompt_lookup_num_tokens=K); greedy search only, off by default)."""
    p.add_argument("--prompt_lookup_num_tokens", type=int, default=None,
                   help="draft up to K ids per step by n-gram lookup in the prompt and the answer so far, verified in one pass "
                        "(greedy search only; the ids are unchanged); needs max_batch >= batch x (K + 1)")
    p.add_argument("--max_matching_ngram_size", type=int, default=None,
                   help="with --prompt_lookup_num_tokens: the longest n-gram matched (default 2)")


def lookup_kwargs(args) -> dict:
    """generate() keywords of add_lookup_args' options (unset or 0: none)."""
    k = getattr(args, "prompt_lookup_num_tokens", None)
    if not k:
        return {}
    kw = {"prompt_lookup_num_tokens": int(k)}
    if getattr(args, "max_matching_ngram_size", None) is not None:
        kw["max_matching_ngram_size"] = int(args.max_matching_ngram_size)
    return kw


def add_constraint_args(p) -> None:
    """The drivers' constrained decoding: answers from a closed vocabulary (generate(prefix_allowed_tokens_fn=TokenTrie))."""
    p.add_argument("--allowed_terms", type=str, default=None,
                   help="file with one allowed answer per line (a GO term, an EC number, a keyword): the output is one of them")
    p.add_argument("--allowed_separator", type=str, default=None,
                   help="with --allowed_terms: the text between two answers of a list (e.g. '; '); unset: exactly one answer")
    p.add_argument("--allowed_prefix", type=str, default="",
                   help="with --allowed_terms: text put in front of every answer before tokenising (most tokenisers encode a "
                        "word differently behind a space)")


def token_constraint(args, tokenizer):
    """The TokenTrie of add_constraint_args' options, built once at start (None when --allowed_terms is unset).  Its end id is
    the tokenizer's EOS id, which the drivers also pass as pad / eos."""
    path = getattr(args, "allowed_terms", None)
    if not path:
        return None
    from .constraint import TokenTrie
    with open(path) as f:
        terms = [line.rstrip("\n") for line in f if line.strip()]
    return TokenTrie.from_strings(tokenizer, terms, end_token_id=tokenizer.eos_token_id,
                                  separator=getattr(args, "allowed_separator", None), prefix=getattr(args, "allowed_prefix", "") or "")
