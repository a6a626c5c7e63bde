"""Host-side parts of generate(prefix=...) that need no GPU: the C ABI additions of both library builds, the snapshot size, the
argument checks that return before any device call, and the offset planning (opus_pllm_amd/prefix.py) against the brute-force
restatement of tests/prefix_generate_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.prefix import CapacityError, plan_prefill_behind, snapshot_bytes
from prefix_generate_ref import brute_groups, brute_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"opus_llama_prefix_bytes": 3, "opus_llama_prefix_export": 8, "opus_llama_prefill_behind": 10, "opus_generate_scored_behind": 20,
       "opus_llama_score_continuations_detached": 13, "opus_llama_score_tree_detached": 28}


@pytest.mark.parametrize("so", ["libopus_pllm.so", "libopus_pllm_bf16.so"])
def test_new_symbols_exported_and_bound(so):
    lib = C.CDLL(os.path.join(ROOT, "opus-pllm_amd", "lib", so))
    header = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in NEW.items():
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name) is not None
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert lib.opus_abi_version() == _cabi.ABI_VERSION == 10            # additive: the version stays
    assert "typedef struct opus_prefix_snap" in header
    # struct opus_prefix_snap: four pointers, two int32
    assert C.sizeof(_cabi.CPrefixSnap) == 4 * C.sizeof(C.c_void_p) + 8
    assert [f[0] for f in _cabi.CPrefixSnap._fields_] == ["d_k", "d_v", "d_kstart", "h_kstart", "P", "Tp"]


def test_prefix_bytes_is_the_closed_form():
    lib = _cabi.lib()
    for cfg in (opa.micro(), opa.micro_qwen(), opa.micro_opt(), opa.llama3_8b(max_batch=64, max_prompt=110, max_new_tokens=16)):
        cc = _cabi.CConfig.from_config(cfg)
        for P, Tp in ((1, 1), (3, 37), (cfg.max_batch, cfg.max_prompt), (2, cfg.max_prompt + cfg.max_new_tokens)):
            want = 2 * cfg.dec_layers * P * cfg.dec_kv_heads * Tp * cfg.dec_head_dim * 2
            assert lib.opus_llama_prefix_bytes(C.byref(cc), P, Tp) == want, (P, Tp)
            assert snapshot_bytes(cfg.dec_layers, cfg.dec_kv_heads, cfg.dec_head_dim, P, Tp) == want
        for P, Tp in ((0, 4), (cfg.max_batch + 1, 4), (1, 0), (1, cfg.max_prompt + cfg.max_new_tokens + 1)):
            assert lib.opus_llama_prefix_bytes(C.byref(cc), P, Tp) == -1, (P, Tp)
    # the headline shape: 64 rows x 40 slots of Llama-3-8B (32 layers, 8 kv heads, head_dim 128) = 335.5 MB
    big = _cabi.CConfig.from_config(opa.llama3_8b(max_batch=64, max_prompt=110, max_new_tokens=16))
    assert lib.opus_llama_prefix_bytes(C.byref(big), 64, 40) == 2 * 32 * 64 * 8 * 40 * 128 * 2
    bad = _cabi.CConfig.from_config(opa.micro())
    bad.dec_heads = 0
    assert lib.opus_llama_prefix_bytes(C.byref(bad), 1, 1) == -1


def test_entries_refuse_null_arguments_before_any_device_call():
    lib = _cabi.lib()
    assert lib.opus_llama_prefix_export(None, 0, 1, 1, None, None, None, None) != 0
    assert lib.opus_llama_prefill_behind(None, None, None, 1, 1, None, None, None, None, None) != 0
    assert lib.opus_generate_scored_behind(None, None, None, 1, 1, None, None, 1, None, 0, 0, 0.0, 1.0, 0, None, None, None, None,
                                           None, None) == -1
    assert lib.opus_llama_score_continuations_detached(None, None, None, 1, 1, None, None, None, None, None, None, 0, None) == -1
    assert lib.opus_llama_score_tree_detached(None, None, None, 0, None, None, None, 0, None, 0, None, None, None, 0, None, None, None,
                                              0, None, 0, None, None, None, None, 1, None, 0, None) == -1


def _check(kstart, Tp, src, lens, n, caps=(64, 4096, 1 << 20)):
    plan = plan_prefill_behind(kstart, Tp, src, lens, n, *caps)
    ref = brute_plan(list(kstart), Tp, list(src), list(lens), n)
    assert plan.T_new == ref["T_new"] == Tp + n
    assert plan.new_kstart.tolist() == ref["new_kstart"]
    assert plan.prefix_slot0.tolist() == ref["prefix_slot0"]
    assert plan.prefix_len.tolist() == ref["prefix_len"]
    assert plan.suffix_slot0.tolist() == ref["suffix_slot0"]
    # rotary / learned position of suffix position t is t - nkst[r]: at t = 0 the number of real prefix tokens
    assert (-plan.nkst).tolist() == ref["pos_suffix0"] == ref["prefix_len"]
    assert plan.pad.tolist() == [n - l for l in lens]
    off, lst = brute_groups(list(src), len(kstart))
    assert plan.off.tolist() == list(off) and plan.list.tolist() == lst
    for r, row in enumerate(ref["rows"]):
        # every row ends at T' - 1 with its last suffix token; the prefix block is contiguous and moved by d_r
        assert row[-1] == ("suffix", lens[r] - 1)
        p, d = src[r], n - lens[r]
        for s in range(kstart[p], Tp):
            assert row[s + d] == ("prefix", s)
        for t in range(lens[r]):
            assert row[Tp + d + t] == ("suffix", t)
    assert plan.src.dtype == plan.lens.dtype == plan.new_kstart.dtype == np.int32
    return plan


def test_plan_named_cases():
    _check([0], 5, [0], [1], 1)                                          # n_r = n = 1
    _check([0, 5, 36], 37, [2, 0, 0, 1, 2, 2, 0], [1, 4, 7, 7, 2, 1, 6], 7)   # repeats, permuted, n_r = 1 and n_r = n
    _check([3, 0, 9, 1], 12, [1, 3], [5, 2], 5)                          # R < P, rows 0 and 2 unused
    _check([2, 0], 8, [0, 1, 1, 0, 0, 1, 0], [3, 3, 1, 2, 3, 3, 1], 3)   # R > P
    _check([0, 0, 0], 40, [0, 1, 2], [9, 9, 9], 9)                       # the identity, nothing padded


def test_plan_random_cases_against_the_restatement():
    rng = np.random.default_rng(7)
    for _ in range(300):
        P, Tp = int(rng.integers(1, 7)), int(rng.integers(1, 70))
        kstart = rng.integers(0, Tp, P)
        R, n = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        src = rng.integers(0, P, R)
        lens = rng.integers(1, n + 1, R)
        if rng.random() < 0.3:
            lens[int(rng.integers(0, R))] = 1
        if rng.random() < 0.3:
            lens[int(rng.integers(0, R))] = n
        _check(kstart.tolist(), Tp, src.tolist(), lens.tolist(), n)


def test_plan_errors():
    ok = dict(kstart=[0, 2], Tp=10, src=[0, 1, 1], lens=[2, 3, 1], n=3, max_batch=4, max_prompt=13, rows_cap=9)
    plan_prefill_behind(**ok)                                            # exactly at every capacity
    with pytest.raises(CapacityError, match="3 decoder rows.*max_batch=2"):
        plan_prefill_behind(**dict(ok, max_batch=2))
    with pytest.raises(CapacityError, match="10 slots.*3 positions = 13.*max_prompt=12"):
        plan_prefill_behind(**dict(ok, max_prompt=12))
    with pytest.raises(CapacityError, match="3 x 3 suffix positions.*hold 8"):
        plan_prefill_behind(**dict(ok, rows_cap=8))
    for bad in (dict(lens=[2, 0, 1]), dict(lens=[2, 4, 1]), dict(src=[0, 2, 1]), dict(src=[0, -1, 1]), dict(lens=[2, 3]),
                dict(src=[], lens=[]), dict(kstart=[0, 10]), dict(n=0)):
        with pytest.raises(ValueError) as e:
            plan_prefill_behind(**dict(ok, **bad))
        assert not isinstance(e.value, CapacityError), bad
    with pytest.raises(ValueError, match="row 1 is empty"):
        plan_prefill_behind(**dict(ok, lens=[2, 0, 1]))
