#!/usr/bin/env python3
"""Interactive annotation loop: the MI355X-native counterpart of eval/run_opus_online.py (one process, one GPU).

  python opus-pllm_amd/eval_online.py --model-base-path <hf dir | synthetic:c1_tiny> --opus-pllm-weights-path <adapter dir>

Per turn (run_opus_online.py:29-92): read an instruction and an optional protein sequence (re-asked until it is empty or
made of the 20 standard residues), build the v0 "Student / Professor" prompt, generate (text-only when no sequence is
given), cut the reply at the first '###', print.  `answer_once` is the loop body, importable for tests and services.
--multi_turn keeps the conversation until the instruction '/new': every later turn is generated behind the kept KV cache of the
turns before it (chat.ChatSession; `chat_once` is that loop body).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import opus_pllm_amd as opa                                                    # noqa: E402
from opus_pllm_amd.builder import load_pretrained_model, return_cstp_path      # noqa: E402
from opus_pllm_amd.conversation import conv_vicuna_v0                          # noqa: E402
from opus_pllm_amd.prompt import (add_constraint_args, add_logits_processor_args, add_lookup_args, add_warper_args,  # noqa: E402
                                  is_protein_sequence, logits_processor_kwargs, lookup_kwargs, online_cut, online_followup,
                                  online_prompt, token_constraint, warper_kwargs)


def answer_once(model, tokenizer, instruction: str, seq: str, args, conv=conv_vicuna_v0, constraint=None):
    """-> (instruction as shown, sequence or None, reply text).  constraint: the TokenTrie of --allowed_terms, if any."""
    dev = model.device
    prompt, shown = online_prompt(instruction, bool(seq), conv)
    if not seq:
        seq = None
        input_ids = torch.as_tensor(tokenizer([prompt]).input_ids).to(dev)
    else:
        input_ids = opa.tokenizer_seq_token(prompt, tokenizer, opa.DEFAULT_SEQ_TOKEN_INDEX, return_tensors="pt").unsqueeze(0).to(dev)
    with torch.inference_mode():
        out = model.generate(input_ids, seq, attention_mask=None, pad_token_id=tokenizer.eos_token_id, seq_embedding=None,
                             do_sample=args.temperature > 0, temperature=args.temperature, top_p=args.top_p,
                             num_beams=args.num_beams, max_new_tokens=args.max_new_tokens, use_cache=True,
                             **logits_processor_kwargs(args), **lookup_kwargs(args), **warper_kwargs(args),
                             **({} if getattr(args, "guidance_scale", None) is None else dict(guidance_scale=args.guidance_scale)),
                             **({} if constraint is None else dict(prefix_allowed_tokens_fn=constraint)))
    text = tokenizer.batch_decode(out, skip_special_tokens=True)[0]
    return shown, seq, online_cut(text, conv.sep)


def _plain_ids(tokenizer, text: str):
    """ids of a text that continues a conversation: no BOS in front"""
    ids = list(tokenizer(text).input_ids)
    return ids[1:] if ids and ids[0] == getattr(tokenizer, "bos_token_id", None) else ids


def chat_once(chat, tokenizer, instruction: str, seq: str, args, conv=conv_vicuna_v0, constraint=None):
    """The loop body of --multi_turn on a chat.ChatSession: '/new' forgets the conversation and returns None; anything else is
    one turn -> (instruction as shown, sequence or None, reply text).  The first turn is answer_once's prompt; a later one feeds
    only what it adds (prompt.online_followup) behind the kept KV cache of everything before it, the answer included.  A protein
    sequence may be given on any turn.  Every turn stops at the separator (stop_sequence), so that the history holds the answer
    and not what the model would write past it."""
    if instruction.strip() == "/new":
        chat.reset()
        return None
    dev = chat.model.device
    stop = _plain_ids(tokenizer, conv.sep.strip())
    first = chat.prefix is None
    if first:
        prompt, shown = online_prompt(instruction, bool(seq), conv)
    else:
        last = chat.turns[-1][1][0].tolist()
        prompt, shown = online_followup(instruction, bool(seq), conv,
                                        after_separator=any(last[i: i + len(stop)] == stop for i in range(len(last))))
    if not seq:
        seq = None
        ids = list(tokenizer(prompt).input_ids) if first else _plain_ids(tokenizer, prompt)
    else:
        ids = opa.tokenizer_seq_token(prompt, tokenizer, opa.DEFAULT_SEQ_TOKEN_INDEX)
        if not first and ids and ids[0] == getattr(tokenizer, "bos_token_id", None):
            ids = ids[1:]
    input_ids = torch.as_tensor([ids], dtype=torch.long).to(dev)
    with torch.inference_mode():
        out = chat.ask(input_ids, seq, attention_mask=None, pad_token_id=tokenizer.eos_token_id, seq_embedding=None,
                       do_sample=args.temperature > 0, temperature=args.temperature, top_p=args.top_p,
                       max_new_tokens=args.max_new_tokens, stop_sequence=stop,
                       **logits_processor_kwargs(args), **warper_kwargs(args),
                       **({} if constraint is None else dict(prefix_allowed_tokens_fn=constraint)))
    text = tokenizer.batch_decode(out.sequences, skip_special_tokens=True)[0]
    return shown, seq, online_cut(text, conv.sep)


def eval_model(args):
    model_name = opa.get_model_name_from_path(args.model_base_path)
    cstp_path = return_cstp_path(args.opus_pllm_weights_path, "modality_encoder/modality_encoding_adapter.ckpt")
    tokenizer, model, _ = load_pretrained_model(args.model_base_path, args.opus_pllm_weights_path, model_name,
                                                args.load_8bit, args.load_4bit, switch_projector_type=args.switch_projector_type,
                                                decoder_weights=getattr(args, "decoder_weights", None),
                                                cstp_path=cstp_path, device="cuda:0",
                                                max_batch=max(1, args.num_beams, 2 if getattr(args, "guidance_scale", None) is not None else 1,
                                                              (getattr(args, "prompt_lookup_num_tokens", None) or 0) + 1),
                                                max_enc_tokens=args.max_residues + 2, max_prompt=args.max_prompt,
                                                max_new_tokens=max(args.max_new_tokens, 1))
    constraint = token_constraint(args, tokenizer)
    chat = opa.ChatSession(model) if getattr(args, "multi_turn", False) else None
    while True:
        try:
            instruction = input("Enter your instruction: ")
            while True:
                seq = input("Enter the protein sequence (or leave empty to skip): ").strip()
                if not seq or is_protein_sequence(seq):
                    print("Valid protein sequence:", seq)
                    break
                print("Invalid sequence!")
        except EOFError:
            return
        if chat is not None:
            turn = chat_once(chat, tokenizer, instruction, seq, args, constraint=constraint)
            if turn is None:
                print("(new conversation)")
                continue
            shown, seq, reply = turn
        else:
            shown, seq, reply = answer_once(model, tokenizer, instruction, seq, args, constraint=constraint)
        print("----------------------------")
        print(f"Instruction: {shown}")
        print(f"Sequence: {seq}")
        print(f"Output: {reply}")
        print("----------------------------")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--model-base-path", type=str, default="synthetic:c1_tiny")
    p.add_argument("--opus-pllm-weights-path", type=str, default="synthetic")
    p.add_argument("--temperature", type=float, default=0.1)
    p.add_argument("--top_p", type=float, default=0.7)
    p.add_argument("--num_beams", type=int, default=1)
    p.add_argument("--max_new_tokens", type=int, default=32)         # run_opus_online.py:101
    p.add_argument("--guidance_scale", type=float, default=None, metavar="G",
                   help="classifier-free guidance against the prompt without its protein (two decoder rows per answer)")
    p.add_argument("--switch_projector_type", type=str, default="mlp2x_gelu")
    p.add_argument("--load-4bit", action="store_true")
    p.add_argument("--decoder_weights", choices=("fp8", "mxfp4"), default=None,
                   help="fp8 / mxfp4: decoder-layer weights also as e4m3 / MXFP4 panels for the decode step (faster decode, 1.5x / 1.27x "
                        "the memory of those weights; mxfp4 is uncalibrated 4-bit rounding: a different model)")
    p.add_argument("--load-8bit", action="store_true")
    p.add_argument("--max_residues", type=int, default=1024)
    p.add_argument("--max_prompt", type=int, default=256)
    p.add_argument("--multi_turn", action="store_true",
                   help="keep the conversation (and its KV cache) across turns until '/new' is entered as the instruction; the whole "
                        "conversation has to fit --max_prompt; greedy / sampling only (no --num_beams, --guidance_scale, prompt lookup)")
    add_logits_processor_args(p)
    add_warper_args(p)
    add_lookup_args(p)
    add_constraint_args(p)
    eval_model(p.parse_args())
