"""CPU-only tests of the sampling warpers (min_p, typical_p, epsilon_cutoff, eta_cutoff): the fp64 reference (warpers_ref.py)
against transformers' own warper classes, generate()'s argument checks before the device, the C-ABI surface, and the share of
draws the reference alone leaves undecided on the GPU test's draw matrix."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
import oracle.sampling as osamp
import warpers_ref as wr
from opus_pllm_amd import _cabi
from opus_pllm_amd.model import OpusLlamaForCausalLM


# ------------------------------------------------------------------------------------------------ the reference against transformers
def _hf_kept(scores64, T, top_p, top_k, min_p, typical_p, eps, eta):
    """Finite set of the installed transformers' warpers chained in GenerationMixin._get_logits_processor's order, in fp64."""
    from transformers.generation import logits_process as lp
    chain = []
    if T != 1.0:
        chain.append(lp.TemperatureLogitsWarper(T))
    if top_k:
        chain.append(lp.TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=1))
    if top_p < 1.0:
        chain.append(lp.TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=1))
    if min_p is not None:
        chain.append(lp.MinPLogitsWarper(min_p=min_p, min_tokens_to_keep=1))
    if typical_p < 1.0:
        chain.append(lp.TypicalLogitsWarper(mass=typical_p, min_tokens_to_keep=1))
    if 0.0 < eps < 1.0:
        chain.append(lp.EpsilonLogitsWarper(epsilon=eps, min_tokens_to_keep=1))
    if 0.0 < eta < 1.0:
        chain.append(lp.EtaLogitsWarper(epsilon=eta, min_tokens_to_keep=1))
    s = torch.from_numpy(scores64)
    for w in chain:
        s = w(None, s)
    return torch.isfinite(s).numpy()


def _rows64(kind, V, B, seed):
    """fp64 rows holding fp32 values (what the reference reads): Gaussian, peaked, all-equal, with -inf entries."""
    return wr.rows(kind, V, B, seed).astype(np.float64)


_SETTINGS = [  # (T, top_p, top_k, min_p, typical_p, epsilon, eta)
    (1.0, 1.0, 0, 0.05, 1.0, 0.0, 0.0), (1.0, 1.0, 0, 0.0, 1.0, 0.0, 0.0), (1.0, 1.0, 0, 1.0, 1.0, 0.0, 0.0),
    (1.0, 1.0, 0, None, 0.2, 0.0, 0.0), (0.7, 1.0, 0, None, 0.9, 0.0, 0.0), (1.0, 1.0, 0, None, 1.0, 3e-3, 0.0),
    (1.0, 1.0, 0, None, 1.0, 0.0, 3e-3), (2.0, 1.0, 0, None, 1.0, 0.0, 0.05),
    (0.7, 0.9, 50, 0.02, 0.9, 3e-4, 3e-4), (1.0, 0.9, 0, 0.02, 0.5, 1e-3, 2e-3), (1.5, 1.0, 50, 0.1, 0.8, 1e-3, 2e-3),
]


@pytest.mark.parametrize("V", [96, 1040, 4000])
def test_reference_keeps_what_transformers_keeps(V):
    """Outside the borderline tokens the reference's kept set is the finite set of transformers' chain: every warper alone, all
    together, min_p in {0, 0.05, 1}; Gaussian sigma 1 / 2 / 4, peaked and -inf rows."""
    n = border = dropped_top = 0
    for kind in ("gauss1", "gauss2", "gauss4", "peaked", "neginf"):
        x = _rows64(kind, V, 4, V + len(kind))
        for T, tp, k, mp, ty, e, h in _SETTINGS:
            hf = _hf_kept(x, T, tp, k, mp, ty, e, h)
            for b in range(x.shape[0]):
                ref = wr.WarpRef(x[b], T, tp, k, mp or 0.0, ty, e, h)
                if ref.tie_cut:               # (the nucleus cut inside a tie: transformers' sort order decides, the project keeps ties together)
                    continue
                assert not (ref.kept & ~hf[b]).any(), (kind, T, tp, k, mp, ty, e, h, b, np.nonzero(ref.kept & ~hf[b])[0])
                assert not (hf[b] & ~ref.maybe).any(), (kind, T, tp, k, mp, ty, e, h, b, np.nonzero(hf[b] & ~ref.maybe)[0])
                n += 1
                border += int(ref.borderline.sum())
                dropped_top += int(not ref.maybe[int(np.argmax(x[b]))])
    assert n >= 200 and border <= n // 10, (n, border)        # (the comparison is not hollow: few tokens are excused)
    assert dropped_top > 0                                      # typical_p did remove the arg-max token somewhere


@pytest.mark.parametrize("V", [96, 1040, 4000])
def test_reference_on_equal_values(V):
    """All-equal rows (top-k / top-p off): min_p and typical_p keep the one tie, and a cutoff above 1 / V removes nothing."""
    x = np.zeros((1, V))
    for mp, ty, e, h in ((0.05, 1.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), (None, 0.5, 0.0, 0.0), (None, 1.0, 2.0 / V, 0.0),
                         (None, 1.0, 0.0, 2.0 / V), (0.5, 0.5, 2.0 / V, 2.0 / V)):
        hf = _hf_kept(x, 1.0, 1.0, 0, mp, ty, e, h)
        ref = wr.WarpRef(x[0], 1.0, 1.0, 0, mp or 0.0, ty, e, h)
        assert hf.all() and ref.kept.all() and not ref.borderline.any(), (V, mp, ty, e, h)


# ------------------------------------------------------------------------------------------------ argument checks, before the device
def _hostless_model():
    m = object.__new__(OpusLlamaForCausalLM)
    m.generation_config = types.SimpleNamespace(pad_token_id=0, eos_token_id=None)
    m.cfg = opa.micro()
    return m


_IDS = torch.ones((1, 4), dtype=torch.long)


@pytest.mark.parametrize("kw,msg", [
    (dict(min_p=-0.1), "`min_p` has to be a float in the [0, 1] interval"), (dict(min_p=1.5), "`min_p` has to be a float in the [0, 1] interval"),
    (dict(min_p="a"), "`min_p` has to be a float"),
    (dict(typical_p=0.0), "`typical_p` has to be a float > 0 and < 1"), (dict(typical_p=1.2), "`typical_p` has to be a float > 0 and < 1"),
    (dict(epsilon_cutoff=1.0), "`epsilon_cutoff` has to be a float > 0 and < 1"), (dict(epsilon_cutoff=-1e-3), "`epsilon_cutoff` has to be a float > 0 and < 1"),
    (dict(eta_cutoff=1.0), "`eta_cutoff` has to be a float > 0 and < 1"), (dict(eta_cutoff=-1e-3), "`eta_cutoff` has to be a float > 0 and < 1")])
def test_bad_values_raise_transformers_messages_before_the_device(kw, msg):
    m = _hostless_model()                    # no library context, no stream: anything that touched the device would fail otherwise
    with pytest.raises(ValueError) as e:
        m.generate(_IDS, do_sample=True, max_new_tokens=2, **kw)
    assert msg in str(e.value)
    with pytest.raises(ValueError) as e:
        m.generate_continuous([torch.tensor([5, 6, 7])], None, max_new_tokens=2, do_sample=True, **kw)
    assert msg in str(e.value)


@pytest.mark.parametrize("kw", [dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=3e-4)])
def test_beams_with_a_warper_raise(kw):
    m = _hostless_model()
    with pytest.raises(NotImplementedError) as e:
        m.generate(_IDS, do_sample=True, num_beams=2, max_new_tokens=2, **kw)
    assert "num_beams" in str(e.value)


def test_off_values_are_off():
    from opus_pllm_amd.model import _sampling_warpers
    for kw in ({}, dict(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None), dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)):
        kw = dict(kw, other=1)
        assert _sampling_warpers(kw) is None and kw == dict(other=1)
    assert _sampling_warpers(dict(min_p=0.05)) == (0.05, 1.0, 0.0, 0.0)
    assert _sampling_warpers(dict(typical_p=0.5, eta_cutoff=1e-3)) == (0.0, 0.5, 0.0, 1e-3)


# ------------------------------------------------------------------------------------------------ C ABI
def test_setter_is_declared_bound_and_refuses_a_null_context():
    assert "opus_set_sampling_warpers" in _cabi.SIGNATURES
    lib = _cabi.lib()
    assert lib.opus_abi_version() == 10
    assert lib.opus_set_sampling_warpers(None, 0.0, 1.0, 0.0, 0.0) == -1          # OPUS_EBADARG, before the device is touched
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opus_pllm.h")).read()
    assert "int opus_set_sampling_warpers(opus_ctx *ctx, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff);" in hdr
    assert "#define OPUS_ABI_VERSION 10" in hdr


# ------------------------------------------------------------------------------------------------ the GPU matrix, the reference alone
@pytest.mark.parametrize("i", range(len(wr.MATRIX)))
def test_matrix_case_is_decisive_enough(i):
    """For every case of test_gpu_warpers' draw matrix the reference alone, at its margins, leaves at most NONDECISIVE_MAX of the
    draws undecided (NONDECISIVE_MAX_PM1E4 on the rows near +-1e4) - a case that excused more would test little on the GPU."""
    V, B, kind, T, tp, k, w, steps, what = wr.MATRIX[i]
    _, refs, draws = wr.case_refs(i)
    nd = sum(int((~d[1]).sum()) for d in draws)
    assert nd <= wr.nondecisive_cap(kind) * B * steps, (what, nd / (B * steps))
    if "arg-max dropped" in what:
        lg = wr.rows(kind, V, B, V + len(kind))
        assert any(not r.maybe[int(np.argmax(l))] for r, l in zip(refs, lg)), what
    if "nothing removed" in what or "all kept" in what:
        assert all(r.kept.all() for r in refs), what
    elif kind != "pm1e4":                      # (the warpers do narrow what top-k / top-p kept; near +-1e4 one or two tokens are left to begin with)
        assert sum(r.maybe.sum() < r.base_kept.sum() for r in refs) >= B // 2, what
    else:
        assert any((r.base_kept & ~r.maybe).any() for r in refs), what


def test_matrix_reaches_all_three_stage2_branches():
    br = set()
    for V, B, kind, T, tp, k, w, steps, _ in wr.MATRIX:
        x = wr.rows(kind, V, 1, V + len(kind))
        br.add(wr.branch(osamp.HeadRef(x[0], T, tp, k).nc))
    assert br == {"exact", "lds", "global"}, br
