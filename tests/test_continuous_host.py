"""CPU-only tests of generate_continuous(): the C-ABI surface, the argument checks and the schedule (continuous.py), which is a
pure function of the prompts' lengths and the answers' lengths."""
import ctypes
import os
import re
import types

import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, continuous as cont
from opus_pllm_amd.model import OpusLlamaForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = {"opus_stream_lag": 0, "opus_stream_begin": 14, "opus_stream_run": 7, "opus_stream_refill": 8, "opus_stream_end": 3,
          "opus_debug_stream_state": 8}


def test_stream_symbols_declared_and_bound_at_abi_10():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "opus_pllm.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for name, nargs in STREAM.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr)
        assert m, name
        declared = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
        assert declared == nargs == len(_cabi.SIGNATURES[name][1]), name
        fn = getattr(lib, name)
        assert fn.argtypes == _cabi.SIGNATURES[name][1]
    assert _cabi.ABI_VERSION == 10 and lib.opus_abi_version() == 10
    assert lib.opus_stream_lag() == cont.LAG
    bf16 = ctypes.CDLL(os.path.join(os.path.dirname(_cabi.LIB_PATH), "libopus_pllm_bf16.so"))
    for name in STREAM:
        assert getattr(bf16, name) is not None
    from importlib import util
    spec = util.spec_from_file_location("_b", os.path.join(ROOT, "opus-pllm_amd", "build.py"))
    b = util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "stream.hip" in b.SOURCES and all(k in b.NO_SCRATCH for k in ("stream_finish_kernel", "stream_refill_kernel"))


def test_null_context_is_refused_without_a_device():
    lib = _cabi.lib()
    t, e = ctypes.c_int32(0), (ctypes.c_int32 * 1)()
    assert lib.opus_stream_run(None, 0, 1, 1, ctypes.byref(t), e, None) == -1
    assert lib.opus_stream_end(None, None, None) == -1
    assert lib.opus_stream_begin(None, None, None, 1, 1, 1, None, 0, 0, 0.0, 1.0, 0, None, None) == -1


def _hostless_model():
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro()
    return m


@pytest.mark.parametrize("kw,name", [
    (dict(num_beams=2), "num_beams"), (dict(num_return_sequences=2), "num_return_sequences"),
    (dict(guidance_scale=1.5), "guidance_scale"), (dict(prefix=object()), "prefix"),
    (dict(prefix_allowed_tokens_fn=lambda b, s: [1]), "prefix_allowed_tokens_fn"),
    (dict(repetition_penalty=1.2), "repetition_penalty"), (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"),
    (dict(bad_words_ids=[[3]]), "bad_words_ids"), (dict(min_length=4), "min_length"), (dict(min_new_tokens=2), "min_new_tokens"),
    (dict(output_scores=True), "output_scores"), (dict(output_logits=True), "output_logits"),
    (dict(output_token_logprobs=True), "output_token_logprobs")])
def test_unsupported_arguments_raise_and_name_themselves(kw, name):
    m = _hostless_model()                   # no library context, no stream: anything that touched the device would fail otherwise
    with pytest.raises(NotImplementedError, match=name):
        m.generate_continuous([torch.tensor([5, 6, 7])], None, max_new_tokens=2, **kw)


def test_capacity_violations_raise_opus_error_2_before_the_device():
    m = _hostless_model()
    p = [torch.tensor([5, 6, 7])]
    for kw in (dict(slots=m.cfg.max_batch + 1), dict(max_new_tokens=m.cfg.max_new_tokens + 1), dict(slots=0)):
        with pytest.raises(_cabi.OpusError) as e:
            m.generate_continuous(p, None, **{"max_new_tokens": 2, **kw})
        assert e.value.code == -2
    with pytest.raises(_cabi.OpusError) as e:
        m.generate_continuous([torch.arange(3, 3 + m.cfg.max_prompt + 1)], None, max_new_tokens=2)
    assert e.value.code == -2
    with pytest.raises(ValueError):
        m.generate_continuous(p, ["A", "C"], max_new_tokens=2)
    with pytest.raises(TypeError):
        m.generate_continuous(p, None, max_new_tokens=2, no_such_option=1)


# ---------------------------------------------------------------------------------------------- the schedule
def _check(lens, n_tok, slots, max_new, S, stats, sim):
    """Invariants of any schedule: every prompt once, inside its session's slots and steps; statistics add up."""
    N = len(lens)
    assert sorted(h[0] for h in sim.harvested) == list(range(N))
    for p, row, start, end in sim.harvested:
        assert end - start + 1 == n_tok[p] <= max_new and 0 <= row < slots
        assert start + max_new <= S and end < S
    assert stats["live_row_steps"] == sum(n_tok)
    begins = [e for e in sim.log if e[0] == "begin"]
    assert stats["rows_refilled"] == sum(len(e[2]) for e in sim.log if e[0] == "refill") + sum(len(e[1]) for e in begins[1:])
    assert stats["rows_refilled"] == N - len(begins[0][1])
    assert stats["refills"] == sum(1 for e in sim.log if e[0] == "refill")
    assert stats["sessions"] == sum(1 for e in sim.log if e[0] == "begin")
    assert stats["decode_steps"] == sum(e[1] for e in sim.log if e[0] == "end")
    assert stats["slot_steps"] >= stats["live_row_steps"]
    T0 = None
    for e in sim.log:
        if e[0] == "begin":
            T0 = e[2]
            assert T0 == max(lens[p] for p in e[1]) and len(e[1]) <= slots
        elif e[0] == "refill":
            for r, p in e[2]:
                assert lens[p] <= T0 + e[1]                       # rule 3: the prompt fits under the session's slots


def test_fit_rules_overtaking_and_input_order():
    # prompt 2 (30 positions) is longer than the first T0 = 10: it waits until 10 + t >= 30 while 3 and 4 overtake it
    lens = [10, 8, 30, 6, 7]
    n_tok = [2, 12, 3, 4, 12]                                       # (prompt 4 keeps the session alive past step 20)
    stats, sim = cont.simulate(lens, n_tok, slots=2, max_new=12, S=40, refill_min=1)
    _check(lens, n_tok, 2, 12, 40, stats, sim)
    assert sim.log[0] == ("begin", (0, 1), 10)
    # row 0 ends at step 1; the host sees it LAG steps later, at boundary 1 + LAG: prompt 3 overtakes prompt 2
    assert sim.log[1] == ("refill", 1 + cont.LAG, ((0, 3),))
    placed = stats["placements"]
    assert placed[3][2] < placed[2][2] or placed[3][0] < placed[2][0]
    assert placed[2] == (0, 1, 20)                                  # 30 positions fit from boundary t = 20 on: row 1 was free
    assert stats["sessions"] == 1 and stats["rows_refilled"] == 3
    # a prompt that never fits inside the session (t + max_new <= S fails before 10 + t reaches it) opens the next session
    lens2 = [10, 8, 45, 6]
    stats2, sim2 = cont.simulate(lens2, [2, 3, 3, 4], slots=2, max_new=12, S=40, refill_min=1)
    _check(lens2, [2, 3, 3, 4], 2, 12, 40, stats2, sim2)
    assert stats2["sessions"] == 2 and stats2["placements"][2] == (1, 0, 0)
    assert stats2["placements"][3][0] == 0                          # prompt 3 overtook it inside the first session


def test_step_budget_ends_a_session_and_drains():
    # S = 40, budget 12: a row may begin at t <= 28 only; 13 full-budget answers on 4 rows need more than one session
    lens = [9] * 13
    n_tok = [12] * 13
    stats, sim = cont.simulate(lens, n_tok, slots=4, max_new=12, S=40, refill_min=1)
    _check(lens, n_tok, 4, 12, 40, stats, sim)
    assert stats["sessions"] >= 2
    for e in sim.log:
        if e[0] == "refill":
            assert e[1] + 12 <= 40
    # equal lengths: the rows end together, so the first refill takes all four rows at once
    assert [len(e[2]) for e in sim.log if e[0] == "refill"][0] == 4


def test_refill_min_waits_for_rows_but_never_blocks():
    lens = [5] * 12
    n_tok = [1, 4, 8, 12, 2, 3, 9, 1, 1, 1, 1, 1]
    s1, sim1 = cont.simulate(lens, n_tok, slots=4, max_new=12, S=64, refill_min=1)
    s3, sim3 = cont.simulate(lens, n_tok, slots=4, max_new=12, S=64, refill_min=3)
    _check(lens, n_tok, 4, 12, 64, s1, sim1)
    _check(lens, n_tok, 4, 12, 64, s3, sim3)
    assert s3["refills"] < s1["refills"] and s3["rows_refilled"] == s1["rows_refilled"] == 8
    sizes3 = [len(e[2]) for e in sim3.log if e[0] == "refill"]
    assert all(n >= 3 for n in sizes3[:-1])                         # (the last one takes what the queue still holds)
    assert cont.default_refill_min(64) == 16 and cont.default_refill_min(3) == 1
    with pytest.raises(ValueError):
        cont.simulate(lens, n_tok, slots=4, max_new=12, S=64, refill_min=0)


def test_schedule_is_a_function_of_the_lengths_and_sees_rows_lag_steps_late():
    lens = [7, 9, 12, 5, 6, 30, 8, 4, 11, 10, 6]
    n_tok = [3, 12, 5, 1, 7, 2, 12, 4, 6, 9, 1]
    a, sa = cont.simulate(lens, n_tok, slots=4, max_new=12, S=40)
    b, sb = cont.simulate(lens, n_tok, slots=4, max_new=12, S=40)
    assert a == b and sa.log == sb.log and sa.harvested == sb.harvested
    _check(lens, n_tok, 4, 12, 40, a, sa)
    # no refill can follow a row's end by less than LAG steps, the last rows included: a session's step count is at least
    # its last end + LAG (the native loop stops within LAG steps of the last row, like generate()'s poll)
    ends = {}
    for p, row, start, end in sa.harvested:
        ends.setdefault(a["placements"][p][0], []).append(end)
    steps = [e[1] for e in sa.log if e[0] == "end"]
    for sess, t in enumerate(steps):
        assert t == min(max(ends[sess]) + cont.LAG, 40)
    for e in sa.log:
        if e[0] == "refill":
            for r, p in e[2]:
                prev = [h for h in sa.harvested if h[1] == r and h[3] < e[1] and a["placements"][h[0]][0] == a["placements"][p][0]]
                assert max(h[3] for h in prev) + cont.LAG <= e[1]
    # a shorter lag sees rows earlier: never more decode steps
    c, _ = cont.simulate(lens, n_tok, slots=4, max_new=12, S=40, lag=1)
    assert c["decode_steps"] <= a["decode_steps"]


def test_stream_stop_mirror():
    # rows began at 0 and 5; ends 2 and -1: at boundary t the host knows step t - LAG
    t, seen = cont.stream_stop(3, 4, 1, 40, [0, 5], [2, -1])
    assert (t, seen) == (2 + cont.LAG, [2, -1])
    t, seen = cont.stream_stop(3, 9, 1, 40, [0, 5], [2, -1])          # t_min holds the run back
    assert (t, seen) == (9, [2, -1])
    t, seen = cont.stream_stop(0, 1, 3, 6, [0, 0], [9, 9])            # t_max
    assert (t, seen) == (6, [-1, -1])
    t, seen = cont.stream_stop(0, 1, 3, 40, [0, 0], [4, 6])           # all done beats an unreachable min_free
    assert (t, seen) == (6 + cont.LAG, [4, 6])
    assert cont.run_args([], [], 5, 10, 12, 40, 4, 1) == (6, 5)       # empty queue: drain
    assert cont.run_args([0], [30], 5, 10, 12, 40, 4, 2) == (20, 2)   # the first boundary at which 30 positions fit
    assert cont.run_args([0], [40], 5, 10, 12, 40, 4, 2) == (6, 5)    # fits only where no budget is left: drain
    assert cont.pick_refill([3, 4, 5], {3: 50, 4: 8, 5: 9}, [2, 0], 4, 10, 12, 40) == [(0, 4), (2, 5)]
    assert cont.pick_refill([4], {4: 8}, [0], 29, 10, 12, 40) == []


def test_eval_driver_flags_and_refusals():
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(ROOT, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    p = ddp.build_parser()
    base = ["--input_path", "x.json", "--save_path", "y.json"]
    a = p.parse_args(base)
    assert a.continuous is False and a.slots is None and a.refill_min is None and a.session_steps is None      # off by default
    a = p.parse_args(base + ["--continuous", "--slots", "16", "--refill_min", "2", "--session_steps", "256"])
    assert a.continuous and (a.slots, a.refill_min, a.session_steps) == (16, 2, 256) and ddp.continuous_refusals(a) == []
    for flags, name in ((["--num_beams", "2"], "--num_beams"), (["--num_return_sequences", "2"], "--num_return_sequences"),
                        (["--guidance_scale", "1.5"], "--guidance_scale"), (["--share_prompt_head"], "--share_prompt_head"),
                        (["--save_logprobs"], "--save_logprobs"), (["--dump_logits", "l.pt"], "--dump_logits"),
                        (["--allowed_terms", "t.txt"], "--allowed_terms"), (["--repetition_penalty", "1.2"], "logits-processor")):
        bad = ddp.continuous_refusals(p.parse_args(base + ["--continuous"] + flags))
        assert any(name in b for b in bad), (flags, bad)
