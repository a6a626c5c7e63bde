"""Host tests (no GPU) of generate()'s logits processors: the CPU restatement (tests/logits_proc_ref.py) against the installed
transformers' processor classes and against the reference's own scores (tests/golden/generate_processors_micro.npz), the C ABI
entries, and the calls that raise."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from opus_pllm_amd.model import OpusLlamaForCausalLM, _logits_processors
import logits_proc_ref as lpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _random_case(g, B, V, t):
    x = torch.randn(B, V, generator=g) * 3                       # both signs
    pool = torch.randint(0, V, (B, 5), generator=g)              # few distinct ids: repeats and recurring n-grams
    hist = pool.gather(1, torch.randint(0, 5, (B, t), generator=g))
    return x, hist


@pytest.mark.parametrize("penalty,ngram,min_new", [(1.3, 0, 0), (0.8, 0, 0), (2.0, 2, 3), (None, 1, 0), (None, 3, 9),
                                                   (1.3, 4, 0), (0.8, 2, 5)])
@pytest.mark.parametrize("t", [0, 1, 4, 11, 30])
def test_restatement_matches_transformers(penalty, ngram, min_new, t):
    pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(100 * t + ngram)
    B, V = 6, 37
    x, hist = _random_case(g, B, V, t)
    eos = [int(hist[0, -1]) if t else 3, 11]
    bad = [[eos[0]], [int(hist[1, -1]) if t else 5], [5, 6], [int(hist[2, -2]) if t > 1 else 1, int(hist[2, -1]) if t else 2, 9],
           [7, 8, 9, 10, 11, 12, 13, 14]]
    for b_ in (None, bad):
        ours = lpr.process(x, hist, eos=eos, penalty=penalty, ngram=ngram, bad=b_, min_new=min_new)
        ref = lpr.hf_process(x, hist, eos=eos, penalty=penalty, ngram=ngram, bad=b_, min_new=min_new)
        assert torch.equal(ours.view(torch.int32), ref.view(torch.int32)), (penalty, ngram, min_new, t, b_)


def test_restatement_reproduces_reference_fixture():
    """The restatement applied to the reference's raw logits, with each row's history = the ids before the step, gives the
    reference's processed scores; their arg-max (lowest index among ties) gives its ids."""
    gp = dict(np.load(os.path.join(GOLD, "generate_processors_micro.npz")))
    T = int(gp["T"])
    tags = sorted({k.split(".")[0] for k in gp if "." in k})
    assert len(tags) == 8
    for tag in tags:
        kw = json.loads(str(gp[tag + ".kw"]))
        eos = kw.get("eos_token_id") or []
        min_new = kw.get("min_new_tokens")
        if min_new is None:
            min_new = max(kw.get("min_length", 0) - T, 0)
        seq = torch.from_numpy(gp[tag + ".sequences"])
        sc, lg = torch.from_numpy(gp[tag + ".scores"]), torch.from_numpy(gp[tag + ".logits"])
        for t in range(seq.shape[1]):
            p = lpr.process(lg[t], seq[:, :t], eos=eos, penalty=kw.get("repetition_penalty"), ngram=kw.get("no_repeat_ngram_size", 0),
                            bad=kw.get("bad_words_ids"), min_new=min_new if eos else 0)
            assert torch.equal(p.view(torch.int32), sc[t].view(torch.int32)), (tag, t)
            am = torch.from_numpy(np.argmax(p.numpy(), axis=1))
            fin = torch.zeros(seq.shape[0], dtype=torch.bool)
            for e in eos:
                fin |= (seq[:, :t] == e).any(1)
            assert torch.equal(am[~fin], seq[~fin, t]), (tag, t)
    # every option of the fixture changes the reference's ids
    plain = gp["plain.sequences"]
    for tag in tags:
        if tag != "plain":
            assert not np.array_equal(gp[tag + ".sequences"], plain), tag


def test_new_symbols_are_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "opus_pllm.h")).read(), flags=re.S)
    lib = _cabi.lib()
    for name, nargs in (("opus_set_logits_processors", 7), ("opus_debug_logits_process", 16)):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _cabi.SIGNATURES and len(_cabi.SIGNATURES[name][1]) == nargs
        fn = getattr(lib, name)
        assert fn.restype == ctypes.c_int and fn.argtypes == _cabi.SIGNATURES[name][1]
    assert lib.opus_abi_version() == 10
    bf = ctypes.CDLL(os.path.join(os.path.dirname(_cabi.LIB_PATH), "libopus_pllm_bf16.so"))
    assert bf.opus_set_logits_processors is not None and bf.opus_debug_logits_process is not None


def test_timing_class_listed_before_xent():
    buf = ctypes.create_string_buffer(512)
    _cabi.check(_cabi.lib().opus_timing_names(buf, 512))
    classes = buf.value.decode().split(";")[0].split(",")
    assert classes[-1] == "xent" and classes[-2] == "logitproc", classes


def test_setter_checks_values_without_a_gpu():
    """opus_set_logits_processors checks its values before anything touches the device (a null context is refused first)."""
    lib = _cabi.lib()
    assert lib.opus_set_logits_processors(None, 1.3, 0, 0, None, None, 0) != 0


def _hostless_model():
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro()
    return m


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[3]]),
                                dict(min_new_tokens=3, eos_token_id=[5]), dict(min_length=40, eos_token_id=5)])
def test_beams_with_processors_raise(kw):
    m = _hostless_model()
    with pytest.raises(NotImplementedError) as e:
        m.generate(torch.ones((1, 4), dtype=torch.long), num_beams=2, max_new_tokens=2, **kw)
    assert "num_beams" in str(e.value)


@pytest.mark.parametrize("kw,msg", [
    (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.2), "repetition_penalty"),
    (dict(repetition_penalty="x"), "repetition_penalty"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"), (dict(min_new_tokens=-2, eos_token_id=3), "min_new_tokens"),
    (dict(min_length=-1, eos_token_id=3), "min_length"), (dict(bad_words_ids=[]), "non-empty list"),
    (dict(bad_words_ids=[3, 4]), "list of non-empty lists"), (dict(bad_words_ids=[[3], []]), "list of non-empty lists"),
    (dict(bad_words_ids=[[-1]]), "ids in"), (dict(bad_words_ids=[[96]]), "ids in"), (dict(bad_words_ids=[["a"]]), "ids in"),
    (dict(bad_words_ids=[[1]] * 257), "at most 256"), (dict(bad_words_ids=[list(range(9))]), "at most 8"),
    (dict(bad_words_ids=[list(range(8))] * 129), "at most 1024"),
])
def test_invalid_values_raise(kw, msg):
    m = _hostless_model()
    with pytest.raises(ValueError) as e:
        m.generate(torch.ones((1, 4), dtype=torch.long), max_new_tokens=2, **kw)
    assert msg in str(e.value), str(e.value)


def test_option_parsing():
    """Defaults and no-ops are off; min_length / min_new_tokens need an EOS id; min_new_tokens wins over min_length."""
    for kw in ({}, dict(repetition_penalty=1.0), dict(repetition_penalty=None, no_repeat_ngram_size=0),
               dict(min_new_tokens=4), dict(min_length=30), dict(min_new_tokens=0)):
        assert _logits_processors(dict(kw), [], 96) is None, kw
    assert _logits_processors(dict(min_new_tokens=0), [5], 96) is None
    assert _logits_processors(dict(repetition_penalty=2), [], 96) == (2.0, 0, None, None, ())
    assert _logits_processors(dict(min_length=30), [5], 96) == (1.0, 0, None, 30, ())
    assert _logits_processors(dict(min_length=30, min_new_tokens=2), [5], 96) == (1.0, 0, 2, 30, ())
    assert _logits_processors(dict(bad_words_ids=[[1, 2], [3]], no_repeat_ngram_size=2), [], 96) == (1.0, 2, None, None, ((1, 2), (3,)))
    kw = dict(repetition_penalty=1.2, other=1)
    _logits_processors(kw, [], 96)
    assert kw == dict(other=1)                              # only its own options are taken
