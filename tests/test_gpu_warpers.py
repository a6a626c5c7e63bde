"""The sampling warpers (min_p, typical_p, epsilon_cutoff, eta_cutoff) on the GPU: every draw of sample_warp_draw_kernel against the
fp64 band of warpers_ref.WarpRef (decisive draws equal the rule's pick, every draw is admissible), the off state (ids and graphs
untouched), and the product call replayed step by step on its own logits."""
import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
import oracle.sampling as osamp
import warpers_ref as wr
from opus_pllm_amd import _cabi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_MODELS = {}


def _model(dev, **kw):
    from opus_pllm_amd.model import OpusLlamaForCausalLM
    from opus_pllm_amd.weights import DeviceWeights
    key = tuple(sorted(kw.items()))
    if key not in _MODELS:
        cfg = opa.micro(**kw)
        _MODELS[key] = OpusLlamaForCausalLM(cfg, DeviceWeights.synthetic(cfg, 0, dev), dev)
    return _MODELS[key]


def _draws(model, logits, T, top_p, top_k, warpers, seed, steps, dev):
    """ids [steps, B] of opus_debug_sample at steps 0 .. steps - 1 with the warpers set."""
    lib = _cabi.lib()
    B = logits.shape[0]
    d = torch.from_numpy(logits).to(dev)
    out = torch.empty(steps, B, dtype=torch.int32, device=dev)
    model._set_top_k(top_k)
    model._set_warpers(warpers)
    try:
        for s in range(steps):
            _cabi.check(lib.opus_debug_sample(model._ctx, d.data_ptr(), B, T, top_p, seed, s, out[s].data_ptr(), None))
    finally:
        model._set_warpers(None)
        model._set_top_k(0)
    return out.cpu().numpy()


def test_warper_draws_match_fp64_band(dev):
    """The draw matrix (warpers_ref.MATRIX): V = 96 / 1040 / 32000 / 128256, every warper alone, typical_p with the arg-max dropped,
    all four behind top-k 50 / top-p 0.9, equal values, -inf entries, rows near +-1e4; all three stage-2 branches with a warper on."""
    from gpu_helpers import record
    branches = set()
    report = []
    for i, (V, B, kind, T, tp, k, w, steps, what) in enumerate(wr.MATRIX):
        logits, refs, draws = wr.case_refs(i)
        ids = _draws(_model(dev, dec_vocab=V, max_batch=B), logits, T, tp, k, w, wr.SEED, steps, dev)
        n = nd = bad = mism = 0
        for b in range(B):
            ref = refs[b]
            branches.add(wr.branch(ref.nc))
            pick, decisive, lo, hi = draws[b]
            got = ids[:, b]
            n += steps
            nd += int((~decisive).sum())
            mism += int((decisive & (got != pick)).sum())
            bad += sum(not ref.admissible(int(g), int(a), int(c)) for g, a, c in zip(got, lo, hi))
        rec = dict(V=V, rows=B, kind=kind, T=T, top_p=tp, top_k=k, warpers=list(w), what=what, draws=n, nondecisive=nd / n,
                   mismatches=mism, inadmissible=bad)
        report.append(rec)
        record("warpers_matrix", rec)
    print("\n".join(str(r) for r in report))
    assert branches == {"exact", "lds", "global"}, branches
    for r in report:
        assert r["mismatches"] == 0 and r["inadmissible"] == 0, r
        assert r["nondecisive"] <= wr.nondecisive_cap(r["kind"]), r


def _micro_batch(model, B):
    import gen_scores_checks as gs
    return gs.batch(model.cfg, B)


def _gen(model, ids, mask, seqs, **kw):
    return model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=8, do_sample=True, seed=77, temperature=1.0,
                          top_k=0, **kw)


def test_off_values_draw_the_same_ids(dev):
    """Explicit off values, and min_p = 0.0 alone, give the ids of the call without the arguments; a warper that is on does not."""
    model = _model(dev)
    ids, mask, seqs = _micro_batch(model, 4)
    plain = _gen(model, ids, mask, seqs).cpu()
    off = _gen(model, ids, mask, seqs, min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0).cpu()
    zero = _gen(model, ids, mask, seqs, min_p=0.0).cpu()
    assert torch.equal(off, plain) and torch.equal(zero, plain)
    on = _gen(model, ids, mask, seqs, min_p=1.0).cpu()                  # min_p = 1: only the most probable token is left
    greedy = model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=8, do_sample=False).cpu()
    assert torch.equal(on, greedy) and not torch.equal(on, plain)
    assert torch.equal(_gen(model, ids, mask, seqs).cpu(), plain)        # and the next call without them is plain again


def test_changing_values_instantiates_no_graph(dev):
    """The captured step holds only whether a warper is on: after the first call with one, other values replay the same graph, and
    the off state keeps its own."""
    model = _model(dev, max_new_tokens=16)
    ids, mask, seqs = _micro_batch(model, 4)
    _gen(model, ids, mask, seqs)
    n_off = model.stat("graph_instantiations")
    _gen(model, ids, mask, seqs, min_p=0.05)
    n_on = model.stat("graph_instantiations")
    assert n_on == n_off + 1
    a = _gen(model, ids, mask, seqs, min_p=0.3).cpu()
    b = _gen(model, ids, mask, seqs, typical_p=0.5, eta_cutoff=1e-3).cpu()
    c = _gen(model, ids, mask, seqs, min_p=0.02, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=3e-4).cpu()
    _gen(model, ids, mask, seqs)
    assert model.stat("graph_instantiations") == n_on, (n_off, n_on, model.stat("graph_instantiations"))
    assert torch.equal(_gen(model, ids, mask, seqs, min_p=0.3).cpu(), a)   # (the values did reach the replayed step)
    assert not (torch.equal(a, b) and torch.equal(b, c))


def _replay(out, T, warpers, seed, nret=1):
    """Every step and row of a generate() output against the reference on the device's own logits: the finite set of out.scores is
    the kept set outside the borderline tokens, the sampled id is admissible and equal to the pick where decisive."""
    seq = out.sequences.cpu().numpy()
    cnt = np.full(seq.shape[0], seq.shape[1])                            # (no EOS id: every position is a draw)
    n = nd = mism = bad = sets = 0
    for t in range(seq.shape[1]):
        lg = out.logits[t].float().cpu().numpy()
        sc = out.scores[t].float().cpu().numpy()
        for b in range(seq.shape[0]):
            if t >= cnt[b]:
                continue
            ref = wr.WarpRef(lg[b], T, 1.0, 0, *warpers)
            fin = np.isfinite(sc[b])
            sets += int((ref.kept & ~fin).any() or (fin & ~ref.maybe).any())
            kept = fin & np.isfinite(lg[b])
            assert np.allclose(sc[b][kept], lg[b][kept] / T, rtol=1e-6, atol=0)
            pick, dec, lo, hi = ref.draw(np.array([osamp.draw_uniform(seed, b, t)[1]]))
            g = int(seq[b, t])
            n += 1
            nd += int(not dec[0])
            mism += int(dec[0] and g != int(pick[0]))
            bad += int(not ref.admissible(g, int(lo[0]), int(hi[0])))
    return dict(warpers=list(warpers), nret=nret, draws=n, nondecisive=nd, mismatches=mism, inadmissible=bad, wrong_sets=sets)


@pytest.mark.parametrize("warpers,nret", [((0.05, 1.0, 0.0, 0.0), 1), ((0.0, 0.3, 0.0, 0.0), 1), ((0.02, 0.9, 3e-4, 3e-4), 1),
                                           ((0.02, 0.9, 3e-4, 3e-4), 2)])
def test_generate_replays_against_the_band(dev, warpers, nret):
    from gpu_helpers import record
    model = _model(dev)
    ids, mask, seqs = _micro_batch(model, 4)
    seed = 20261021
    names = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
    out = model.generate(ids, seqs, attention_mask=mask, pad_token_id=2, max_new_tokens=8, do_sample=True, seed=seed, temperature=1.0,
                         top_k=0, num_return_sequences=nret, return_dict_in_generate=True, output_logits=True, output_scores=True,
                         **dict(zip(names, warpers)))
    assert out.sequences.shape[0] == 4 * nret
    rec = _replay(out, 1.0, warpers, seed, nret)
    record("warpers_generate", rec)
    print(rec)
    assert rec["draws"] > 0 and rec["mismatches"] == 0 and rec["inadmissible"] == 0 and rec["wrong_sets"] == 0, rec
    # 32 or 64 draws: one undecided draw is already 3 % of a case, so the matrix's 2 % cannot be asked of it; 10 % - three draws
    # of 32 - still leaves the pick-equality check on nine draws in ten
    assert rec["nondecisive"] <= 0.10 * rec["draws"], rec


def test_generate_continuous_takes_the_warpers(dev):
    """The session's head is the same: with min_p = 1 only the most probable token is left, so the sampled answers are the greedy
    ones; without it they are not."""
    import continuous_checks as cc
    model = _model(dev, max_new_tokens=cc.E2E_S, max_prompt=cc.E2E_MAX_PROMPT)
    prompts, seqs = cc.e2e_prompts(model.cfg, 3)
    prompts, seqs = prompts[:5], seqs[:5]                                 # (four slots: one refill)
    kw = dict(max_new_tokens=6, pad_token_id=2, slots=4)
    greedy = model.generate_continuous(prompts, seqs, **kw)
    plain = model.generate_continuous(prompts, seqs, do_sample=True, seed=5, temperature=1.0, top_k=0, **kw)
    top = model.generate_continuous(prompts, seqs, do_sample=True, seed=5, temperature=1.0, top_k=0, min_p=1.0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(top, greedy))
    assert not all(torch.equal(a, b) for a, b in zip(plain, greedy))
    again = model.generate_continuous(prompts, seqs, do_sample=True, seed=5, temperature=1.0, top_k=0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(again, plain))          # the setting does not outlive its call


def test_session_first_step_draws_what_generate_draws(dev):
    """typical_p, epsilon and eta through the session (opus_stream_begin's upload and plan): the session exports no logits, but its
    step 0 is generate()'s step 0 - the first `slots` prompts are prefilled as one left-padded batch and row r draws with
    (seed, r, 0) in both - so their first ids must be generate()'s with the same warpers (replayed against the band above)."""
    import continuous_checks as cc
    model = _model(dev, max_new_tokens=cc.E2E_S, max_prompt=cc.E2E_MAX_PROMPT)
    prompts, seqs = cc.e2e_prompts(model.cfg, 3)
    prompts, seqs = prompts[:5], seqs[:5]
    ids, mask = cc.left_pad([p.tolist() for p in prompts[:4]])
    firsts = {}
    for seed in (5, 6, 7, 8):
        for w in ({}, dict(typical_p=0.3), dict(min_p=0.02, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=3e-4),
                  dict(typical_p=0.5, epsilon_cutoff=2e-3, eta_cutoff=5e-3)):
            kw = dict(do_sample=True, seed=seed, temperature=1.0, top_k=0, pad_token_id=2, **w)
            want = model.generate(ids, seqs[:4], attention_mask=mask, max_new_tokens=1, **kw).cpu()[:, 0]
            got = model.generate_continuous(prompts, seqs, max_new_tokens=4, slots=4, **kw)
            assert [int(s[0]) for s in got[:4]] == want.tolist(), (seed, w, got, want)
            firsts[seed, tuple(sorted(w))] = want.tolist()
    # (the session did see the setting: typical_p = 0.3 drops the most probable token, so some first id differs from the plain one)
    assert any(firsts[seed, ("typical_p",)] != firsts[seed, ()] for seed in (5, 6, 7, 8)), firsts


def test_generate_from_tokens_does_not_inherit_the_warpers(dev):
    """generate_from_tokens(sampler=...) takes no warper arguments: behind a generate() call with one on it draws the plain ids."""
    from opus_pllm_amd.alphabet import batch_convert_packed
    model = _model(dev)
    ids, mask, seqs = _micro_batch(model, 4)
    toks, cu = batch_convert_packed(seqs)
    d_toks = torch.from_numpy(toks).to(dev)

    def tokens_call():
        return model.generate_from_tokens(d_toks, [int(v) for v in cu], ids.to(dev), mask.to(dev), 8, (), 2, "packed",
                                          sampler=(1.0, 1.0, 77, 0)).cpu()

    plain = _gen(model, ids, mask, seqs).cpu()
    assert torch.equal(tokens_call(), plain)
    on = _gen(model, ids, mask, seqs, min_p=0.3, typical_p=0.5).cpu()
    assert not torch.equal(on, plain)
    assert torch.equal(tokens_call(), plain)
