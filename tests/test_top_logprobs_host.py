"""CPU tests of top log-probs: the fp64 restatement (tests/top_logprobs_ref.py) against torch.topk and the stable sort, the
argument checks of generate() / forward() / generate_continuous(), and the C ABI declarations."""
import os
import re
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.model import OpusLlamaForCausalLM, _top_logprobs_arg, TOP_LOGPROBS_MAX
import top_logprobs_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_equals_torch_topk_without_ties():
    g = torch.Generator().manual_seed(0)
    for V, k in ((96, 20), (1043, 5), (32000, 1), (128256, 20)):
        x = torch.randn(4, V, generator=g, dtype=torch.float64)
        assert all(len(np.unique(r)) == V for r in x.numpy())
        ids, lp, lse = tref.top_logprobs_ref(x.numpy(), k)
        val, idx = torch.topk(x, k, dim=1)
        assert np.array_equal(ids, idx.numpy())
        np.testing.assert_allclose(lp, (val - torch.logsumexp(x, dim=1, keepdim=True)).numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(lse, torch.logsumexp(x, dim=1).numpy(), rtol=0, atol=1e-12)
        f_ids, f_lp, _ = tref.top_logprobs_fast(x.numpy(), k)
        assert np.array_equal(f_ids, ids) and np.array_equal(f_lp, lp)


def test_reference_on_constructed_ties():
    x = np.array([[1.0, 3.0, 3.0, -np.inf, 3.0, 0.0, -0.0, 2.0, -np.inf, 2.0]], dtype=np.float32)
    ids, lp, _ = tref.top_logprobs_ref(x, 10)
    assert ids[0].tolist() == [1, 2, 4, 7, 9, 0, 5, 6, 3, 8]                 # equal values lower id first, -0 == +0, -inf last
    assert np.isneginf(lp[0, 8:]).all() and np.isfinite(lp[0, :8]).all()
    assert np.array_equal(tref.top_ids_fast(x, 10), ids) and np.array_equal(tref.top_ids_fast(x, 4), ids[:, :4])
    g = np.random.default_rng(1)
    t = g.integers(0, 4, (6, 4099)).astype(np.float32)                      # ties everywhere
    for k in (1, 5, 20):
        ids, lp, _ = tref.top_logprobs_ref(t, k)
        assert np.array_equal(ids, np.stack([np.argsort(-r, kind="stable")[:k] for r in t]))
        assert np.array_equal(tref.top_ids_fast(t, k), ids)
    h = torch.randn(3, 5000, generator=torch.Generator().manual_seed(2)).half()   # fp16 rows tie by themselves
    ids, _, _ = tref.top_logprobs_ref(h.numpy(), 20)
    assert np.array_equal(ids, np.stack([np.argsort(-r.astype(np.float32), kind="stable")[:20] for r in h.numpy()]))
    eq = np.full((2, 777), 0.5, dtype=np.float32)
    ids, lp, _ = tref.top_logprobs_ref(eq, 7)
    assert (ids == np.arange(7)).all()
    np.testing.assert_allclose(lp, -np.log(777), atol=1e-12)


def test_argument_values():
    assert _top_logprobs_arg(None, 96) == 0 and _top_logprobs_arg(1, 96) == 1 and _top_logprobs_arg(np.int64(20), 96) == 20
    assert TOP_LOGPROBS_MAX == tref.K_MAX == 20
    for bad in (0, -1, 21, 2.0, "3", True, [3]):
        with pytest.raises(ValueError, match="top_logprobs"):
            _top_logprobs_arg(bad, 96)
    with pytest.raises(ValueError, match="vocabulary"):
        _top_logprobs_arg(9, 8)


def _shell():
    """A model object without a context: the argument checks run before the device is touched."""
    m = OpusLlamaForCausalLM.__new__(OpusLlamaForCausalLM)
    m.cfg = opa.micro()
    m.default_top_k = 50
    m.generation_config = types.SimpleNamespace(pad_token_id=2, eos_token_id=None)
    m.set_stop_sequence = lambda ids: None
    return m


def test_generate_argument_errors():
    m = _shell()
    ids = torch.ones((2, 4), dtype=torch.long)
    for bad in (0, 21, 2.5, "5", 97):
        with pytest.raises(ValueError, match="top_logprobs"):
            m.generate(ids, return_dict_in_generate=True, top_logprobs=bad)
    with pytest.raises(ValueError, match="top_logprobs"):                       # (the value is checked with or without the output object)
        m.generate(ids, top_logprobs=0)
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(ids, return_dict_in_generate=True, top_logprobs=5, num_beams=2)
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        m.generate(ids, return_dict_in_generate=True, top_logprobs=5, prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="top_logprobs"):
        m.generate_continuous([torch.ones(3, dtype=torch.long)], top_logprobs=5)
    assert "top_logprobs" in OpusLlamaForCausalLM._CONTINUOUS_UNSUPPORTED


def test_forward_argument_errors():
    m = _shell()
    ids = torch.ones((2, 4), dtype=torch.long)
    for bad in (0, 21, 1.5, 97):
        with pytest.raises(ValueError, match="top_logprobs"):
            m.forward(ids, labels=ids, top_logprobs=bad)
    with pytest.raises(ValueError, match="labels"):
        m.forward(ids, top_logprobs=5)


def test_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    for name, nargs in (("opus_set_gen_top_logprobs", 4), ("opus_debug_top_logprobs", 11)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_cabi.SIGNATURES[name][1]), name
    lib = _cabi.lib()
    assert lib.opus_abi_version() == 10
    assert lib.opus_set_gen_top_logprobs(None, 5, None, None) == -1             # null context: refused before anything is touched
    assert lib.opus_debug_top_logprobs(None, None, 1, 8, 1, 8, 1, None, None, None, None) == -1
    declared = set(re.findall(r"^(?:int|int32_t|int64_t|const char \*)\s*(opus_\w+)\(", hdr, flags=re.M))
    assert declared == set(_cabi.SIGNATURES), declared ^ set(_cabi.SIGNATURES)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"{len(_cabi.SIGNATURES)} `extern \"C\"` symbols" in readme


def test_timing_class_and_scratch_check():
    import ctypes
    buf = ctypes.create_string_buffer(512)
    _cabi.check(_cabi.lib().opus_timing_names(buf, 512))
    classes = buf.value.decode().split(";")[0].split(",")
    assert "topk" in classes and classes[-1] == "xent", classes
    import importlib.util
    spec = importlib.util.spec_from_file_location("_opus_build_t", os.path.join(ROOT, "opus-pllm_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "topk.hip" in b.SOURCES
    for kern in ("topk_part_kernel", "topk_merge_kernel", "topk_row_lse_kernel"):
        assert kern in b.NO_SCRATCH
    b.build(verbose=False)                                                        # (nothing to do after build(); the remarks sit beside the objects)
    for tag in ("", ".bf16"):
        ru =b.resource_usage(open(os.path.join(b.OBJ, "topk.hip" + tag + ".o.ru.txt")).read())
        names = [n for n in ru if "topk_" in n]
        assert len(names) == 6, names                                             # three kernels, two input types
        for n in names:
            assert ru[n]["ScratchSize [bytes/lane]"] == 0 and ru[n].get("VGPRs Spill", 0) == 0, (n, ru[n])
