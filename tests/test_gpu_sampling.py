"""The sampling head draw by draw: every token sample_stage1_kernel / sample_stage2_kernel (and beam_sample_kernel) draw is checked
against the fp64 restatement in oracle.sampling (HeadRef, beam_reference).  The draw is a pure function of (seed, row, step), so
the host rebuilds each uniform and names the token the rule picks; a draw is "decisive" when no perturbation within the stated
per-token margins (oracle/sampling.py) changes that token.  Decisive draws must match exactly; every draw must be a token the
reference keeps under some admissible perturbation, next to its uniform.  Each case records its counts with gpu_helpers.record.
"""
import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
import oracle.sampling as osamp
from opus_pllm_amd import _cabi

pytestmark = pytest.mark.gpu

NONDECISIVE_MAX = 0.02        # per case
NONDECISIVE_MAX_PM1E4 = 0.10  # rows near +-1e4: the exponent's fp32 rounding, 2^-23 (|l| + |max|) / T, is 2.4e-2 at temperature 0.1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_MODELS = {}


def _model(V, B, dev):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    key = (V, B)
    if key not in _MODELS:
        cfg = opa.micro(dec_vocab=V, max_batch=B)
        _MODELS[key] = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    return _MODELS[key]


def _rows(kind, V, B, seed):
    r = np.random.default_rng(seed)
    if kind.startswith("gauss"):
        x = r.standard_normal((B, V)) * float(kind[5:])
    elif kind == "peaked":                                  # one logit far above the rest
        x = r.standard_normal((B, V)) * 2.0
        x[np.arange(B), r.integers(0, V, B)] += 12.0
    elif kind == "flat":                                    # all equal: nc = V (0: p = 1 exactly, every sum exact)
        x = np.zeros((B, V))
    elif kind == "tie50":                                   # the 50th value tied three more times
        x = r.standard_normal((B, V)) * 2.0
        for b in range(B):
            o = np.argsort(-x[b])
            x[b, o[50:53]] = x[b, o[49]]
    elif kind == "neginf":                                  # -inf entries, and whole parts of them
        x = r.standard_normal((B, V)) * 2.0
        x[r.random((B, V)) < 0.3] = -np.inf
        x[:, : int(0.4 * V)] = -np.inf
    elif kind == "pm1e4":                                   # rows near +1e4 and -1e4
        x = r.standard_normal((B, V)) + np.where(np.arange(B) % 2 == 0, 1e4, -1e4)[:, None]
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


# (V, max_batch = rows, row kind, temperature, top_p, top_k, steps)
CASES = [
    (96, 8, "gauss2", 0.7, 0.9, 0, 256), (96, 8, "gauss2", 2.0, 1.0, 0, 256), (96, 8, "tie50", 1.0, 1.0, 50, 256),
    (96, 8, "peaked", 0.1, 0.7, 50, 256),
    (1040, 128, "gauss2", 0.1, 0.7, 50, 16), (1040, 128, "gauss2", 1.0, 1.0, 0, 16), (1040, 128, "flat", 0.7, 1.0, 0, 16),
    (1040, 128, "neginf", 1.0, 0.9, 0, 16), (1040, 128, "pm1e4", 0.1, 0.7, 50, 16), (1040, 128, "gauss2", 2.0, 0.7, 2000, 16),
    (32000, 16, "gauss5", 1.0, 0.7, 0, 128), (32000, 16, "gauss2", 0.1, 0.7, 50, 128), (32000, 16, "tie50", 0.7, 0.9, 50, 128),
    (50272, 16, "gauss4", 1.0, 0.7, 2000, 128), (50272, 16, "peaked", 1.0, 0.9, 1, 128), (50272, 16, "flat", 1.0, 1.0, 0, 128),
    (128256, 16, "gauss4", 1.0, 0.9, 0, 128), (128256, 16, "flat", 1.0, 1.0, 0, 128), (128256, 16, "neginf", 0.7, 0.7, 128256, 128),
    (128256, 16, "pm1e4", 0.1, 0.7, 50, 128),
    (152064, 16, "gauss6", 1.0, 0.9, 0, 128), (152064, 16, "pm1e4", 0.1, 0.7, 0, 128), (152064, 16, "gauss4", 2.0, 0.9, 50, 128),
]


def _branch(nc):
    return "exact" if nc <= osamp.EXACT_CAP else ("lds" if nc <= osamp.LDS_CAP else "global")


def _draws(model, logits, T, top_p, top_k, seed, steps, dev):
    """ids [steps, B] of opus_debug_sample at steps 0 .. steps - 1."""
    lib = _cabi.lib()
    B = logits.shape[0]
    d = torch.from_numpy(logits).to(dev)
    out = torch.empty(steps, B, dtype=torch.int32, device=dev)
    model._set_top_k(top_k)
    for s in range(steps):
        _cabi.check(lib.opus_debug_sample(model._ctx, d.data_ptr(), B, T, top_p, seed, s, out[s].data_ptr(), None))
    model._set_top_k(0)
    return out.cpu().numpy()


def test_sampling_head_draws_match_fp64_rule(dev):
    """(a) The kernel matrix: six vocabularies (1040: 12 empty parts - a context's vocabulary is a multiple of 16; 152064: 10 values per
    stage-1 thread),
    a 128-row grid, T in {0.1, 0.7, 1, 2}, top_p in {0.7, 0.9, 1}, top_k in {0, 1, 50, >= nc, V}, Gaussian / peaked / flat / tied /
    -inf / +-1e4 rows; all three stage-2 branches (exact rank, bisection in LDS, bisection from global memory)."""
    from gpu_helpers import record
    seed = 0x5EED
    branches = set()
    report = []
    for V, B, kind, T, tp, k, steps in CASES:
        model = _model(V, B, dev)
        logits = _rows(kind, V, B, V + len(kind))
        ids = _draws(model, logits, T, tp, k, seed, steps, dev)
        n = nd = bad = mism = 0
        for b in range(B):
            ref = osamp.HeadRef(logits[b], T, tp, k)
            branches.add(_branch(ref.nc))
            u = np.array([osamp.draw_uniform(seed, b, s)[1] for s in range(steps)])
            pick, decisive, lo, hi = ref.draw(u)
            got = ids[:, b]
            n += steps
            nd += int((~decisive).sum())
            mism += int((decisive & (got != pick)).sum())
            bad += sum(not ref.admissible(int(g), int(a), int(c)) for g, a, c in zip(got, lo, hi))
        rec = dict(V=V, rows=B, kind=kind, T=T, top_p=tp, top_k=k, draws=n, nondecisive=nd / n, mismatches=mism, inadmissible=bad)
        report.append(rec)
        record("sampling_matrix", rec)
    print("\n".join(str(r) for r in report))
    assert branches == {"exact", "lds", "global"}, branches
    for r in report:
        assert r["mismatches"] == 0 and r["inadmissible"] == 0, r
        assert r["nondecisive"] <= (NONDECISIVE_MAX_PM1E4 if r["kind"] == "pm1e4" else NONDECISIVE_MAX), r


@pytest.mark.parametrize("T,top_p,top_k", [(0.1, 0.7, 50), (1.0, 0.9, 50)])
def test_sampling_head_boundary_draws(dev, T, top_p, top_k):
    """(b) Draws aimed at the CDF's ends and boundaries (seed_for_uniform): grid points 0 .. 7 must give the first kept token in index
    order, 2^24 - 8 .. 2^24 - 1 the last one (64 rows), and the two grid points around every interior boundary (8 rows) the token on
    its left or on its right - never another id, never -1.  (Before the draw's interval bounds were made monotone, threads without kept mass could own
    an ulp-wide interval near the total and write -1.)"""
    from gpu_helpers import record
    V, B, step = 32000, 64, 3
    model = _model(V, B, dev)
    logits = _rows("gauss2", V, B, 7)
    lib = _cabi.lib()
    d = torch.from_numpy(logits).to(dev)
    plan = []
    refs = [osamp.HeadRef(logits[b], T, top_p, top_k) for b in range(B)]
    for b, ref in enumerate(refs):
        ks = list(range(8)) + list(range(osamp.U24 - 8, osamp.U24))
        for f in (ref.boundaries() if b < 8 else ()):
            kb = int(np.floor(f * osamp.U24))
            ks += [kb, kb + 1]
        plan += [(b, kk) for kk in ks if 0 <= kk < osamp.U24]
    out = torch.empty(len(plan), B, dtype=torch.int32, device=dev)
    model._set_top_k(top_k)
    for i, (b, kk) in enumerate(plan):
        _cabi.check(lib.opus_debug_sample(model._ctx, d.data_ptr(), B, T, top_p, osamp.seed_for_uniform(kk, b, step), step,
                                          out[i].data_ptr(), None))
    model._set_top_k(0)
    got = out.cpu().numpy()
    wrong = neg = ends = 0
    for i, (b, kk) in enumerate(plan):
        ref, g = refs[b], int(got[i, b])
        pick, dec, lo, hi = ref.draw(np.array([kk / osamp.U24]))
        neg += g < 0
        ok = ref.admissible(g, int(lo[0]), int(hi[0])) and (not dec[0] or g == int(pick[0]))
        kept = np.nonzero(ref.kept)[0]
        if kk < 8 or kk >= osamp.U24 - 8:
            want = kept[0] if kk < 8 else kept[-1]
            ends += 1
            ok &= g == want or not dec[0]
        wrong += not ok
    rec = dict(T=T, top_p=top_p, top_k=top_k, draws=len(plan), end_draws=ends, wrong=wrong, minus_one=neg)
    record("sampling_boundary", rec)
    print(rec)
    assert wrong == 0 and neg == 0, rec


@pytest.mark.parametrize("T,top_p,top_k", [(0.1, 0.7, 50), (1.0, 1.0, 0), (1.0, 0.9, 50)])
def test_generate_sampled_ids_match_fp64_rule(dev, T, top_p, top_k):
    """(c) generate(do_sample=True) at Llama-3-8B widths, 2 layers, batch 64: every sampled id at a counted position against the fp64
    rule on that step's logits (out.logits[t]); the draw of position t uses step t (the step counter starts at 0 with the first
    token and advances once per decode step)."""
    from gpu_helpers import record
    import gen_scores_checks as gs
    cfg = gs.llama8b_shape(64, 2, 4)
    model = _MODELS.get("llama8b") or gs.make_model(cfg, dev)
    _MODELS["llama8b"] = model
    ids, mask, seqs = gs.batch(cfg, 64)
    seed = 20261016
    o = model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=4, do_sample=True, seed=seed, temperature=T,
                       top_p=top_p, top_k=top_k, return_dict_in_generate=True, output_logits=True,
                       output_token_logprobs=True)
    seq, cnt = o.sequences.cpu().numpy(), o.n_tokens.cpu().numpy()
    n = nd = mism = bad = 0
    for t in range(seq.shape[1]):
        lg = o.logits[t].float().cpu().numpy()
        for b in range(seq.shape[0]):
            if t >= cnt[b]:
                continue
            ref = osamp.HeadRef(lg[b], T, top_p, top_k)
            pick, dec, lo, hi = ref.draw(np.array([osamp.draw_uniform(seed, b, t)[1]]))
            g = int(seq[b, t])
            n += 1
            nd += int(not dec[0])
            mism += int(dec[0] and g != int(pick[0]))
            bad += int(not ref.admissible(g, int(lo[0]), int(hi[0])))
    rec = dict(T=T, top_p=top_p, top_k=top_k, draws=n, nondecisive=nd / max(n, 1), mismatches=mism, inadmissible=bad)
    record("sampling_generate", rec)
    print(rec)
    assert n > 0 and mism == 0 and bad == 0, rec
    assert nd < n, rec


@pytest.mark.parametrize("V,K", [(96, 2), (96, 4), (128256, 2), (128256, 4)])
def test_beam_sample_matches_fp64_gumbel_top_m(dev, V, K):
    """(d) opus_beam_sample_topk: on decisive rows the M = 2K flat ids equal the fp64 Gumbel top-M of the kept keys, in order."""
    from gpu_helpers import record
    M, B = 2 * K, 4
    model = _model(V, B * K, dev)
    lib = _cabi.lib()
    r = np.random.default_rng(V + K)
    logits = (r.standard_normal((B * K, V)) * 2.0).astype(np.float32)
    run = np.tile(np.linspace(0.0, -1.5, K), B).astype(np.float32)
    d, d_run = torch.from_numpy(logits).to(dev), torch.from_numpy(run).to(dev)
    sc = torch.empty(B, M, dtype=torch.float32, device=dev)
    ix = torch.empty(B, M, dtype=torch.int32, device=dev)
    n = nd = mism = 0
    for T, tp, k in ((1.0, 0.9, 50), (0.1, 0.7, 50), (1.0, 1.0, 0)):
        model._set_top_k(k)
        refs = [osamp.HeadRef(logits[i], T, tp, k, min_keep=M // K) for i in range(B * K)]
        for step in range(8):
            _cabi.check(lib.opus_beam_sample_topk(model._ctx, d.data_ptr(), d_run.data_ptr(), B, K, M, T, tp, 99, step, sc.data_ptr(),
                                                  ix.data_ptr(), None))
            got = ix.cpu().numpy()
            for b in range(B):
                want, dec = osamp.beam_reference(logits[b * K:(b + 1) * K], run[b * K:(b + 1) * K], T, tp, k, M, 99, step, b,
                                                 refs[b * K:(b + 1) * K])
                n += 1
                nd += int(not dec)
                mism += int(dec and not np.array_equal(got[b], want))
    model._set_top_k(0)
    rec = dict(V=V, K=K, M=M, rows=n, nondecisive=nd / n, mismatches=mism)
    record("beam_sample", rec)
    print(rec)
    assert mism == 0 and nd <= n // 4, rec
