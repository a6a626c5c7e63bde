"""CPU side of the prefill-attention form tests (tests/test_gpu_attn_forms.py): the reference against torch's own attention,
the premises of the peaked input family, the case table against the restated tiling and launcher rule, and the new entry's
binding and argument checks."""
import ctypes as C
import os

import pytest
import torch

from opus_pllm_amd import _cabi
import attn_forms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def peaked():
    """(inputs, reference) of the peaked family per case and operand type, computed once."""
    out = {}
    for dt in (torch.float16, torch.bfloat16):
        for c in R.CASES:
            inp = R.make_inputs(c, "peaked", dt)
            out[c.name, dt] = (inp, R.reference_case(c, inp))
    return out


@pytest.mark.parametrize("name", ["packed_hd16_qt1_trim1", "padded_hd16_qt1_T130", "dec_hd64_qt2"])
def test_reference_matches_torch_sdpa(name):
    """One case of each form: `reference` against scaled_dot_product_attention in fp64 on an explicit boolean mask, on every
    row with a visible key; the others are zero."""
    case = R.CASE_BY_NAME[name]
    inp = R.make_inputs(case, "random")
    ref = R.reference_case(case, inp)
    dark = 0
    for b, (q, k, v) in enumerate(inp["rows"]):
        n = case.row_len(b)
        k0, k1 = case.key_range(b)
        j = torch.arange(n)
        mask = ((j >= k0) & (j < k1))[None, :] & ((j[None, :] <= j[:, None]) if case.causal else torch.ones(n, n, dtype=torch.bool))
        qq = q.double().transpose(0, 1)
        kk = k.double().transpose(0, 1).repeat_interleave(case.group, 0)
        vv = v.double().transpose(0, 1).repeat_interleave(case.group, 0)
        want = torch.nn.functional.scaled_dot_product_attention(qq, kk, vv, attn_mask=mask, scale=case.scale).transpose(0, 1)
        out, computed, has_key, P = ref[b]
        assert torch.equal(has_key, mask.any(-1))
        assert torch.equal(computed, (j >= 1) & (j < n - 1) if case.trim else torch.ones(n, dtype=torch.bool))
        assert float((out[has_key] - want[has_key]).abs().max()) < 1e-12
        assert float(out[~has_key].abs().sum()) == 0.0
        assert float((P.sum(-1)[:, has_key] - 1).abs().max()) < 1e-12
        dark += int((~has_key).sum())
    assert (dark > 0) == (case.form == "decoder")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_peaked_family_premises(peaked, dt):
    """Every checked query's reference mass on pi(i) is at least 0.99 in both operand types (so O[i] = V[pi(i)] up to rounding),
    pi aims only at visible keys, reaches the first visible key, the row's last key and both sides of every 64-key tile boundary,
    and the operands stay finite and far inside the 16-bit range."""
    worst = 1.0
    for c in R.CASES:
        inp, ref = peaked[c.name, dt]
        mass = R.peaked_mass(c, inp, ref)
        assert mass >= R.MASS_MIN, (c.name, mass)
        worst = min(worst, mass)
        assert R.pi_misses(c, inp) == [], c.name
        body = inp["qkv"][:c.rows].float()
        assert bool(torch.isfinite(body).all()) and float(body.abs().max()) < 128, c.name
        assert bool(torch.isnan(inp["qkv"][c.rows:].float()).all())
        for b in range(c.B):
            k0, k1 = c.key_range(b)
            pi = inp["pi"][b]
            i = torch.arange(c.row_len(b))[None, :].expand_as(pi)
            aimed = pi >= 0
            assert bool(((pi >= k0) & (pi < k1))[aimed].all())
            if c.causal:
                assert bool((pi <= i)[aimed].all()) and bool((aimed == (i >= k0)).all())
            else:
                assert bool(aimed.all())
                assert sorted(pi[0, :k1].tolist()) == list(range(k1))          # a permutation of the visible keys
    print("smallest mass", dt, worst)


def test_case_table_reaches_every_cell():
    reached = set()
    for c in R.CASES:
        cells = R.geometry_cells(c)
        assert cells <= set(R.ALL_CELLS), (c.name, cells - set(R.ALL_CELLS))
        reached |= cells
    assert reached == set(R.ALL_CELLS), sorted(set(R.ALL_CELLS) - reached)
    assert len(set(R.ALL_CELLS)) == len(R.ALL_CELLS) == 35
    # the trimmed block counts the table relies on: 66 / 67 tokens at 64 queries per block, 130 / 131 at 128
    for qt, a, b in ((1, 66, 67), (2, 130, 131)):
        QB = 64 * qt
        assert R.cdiv(a - 2, QB) == R.cdiv(a, QB) - 1 and R.cdiv(b - 2, QB) == R.cdiv(b, QB) and (b - 2) % QB == 1
        assert a in R.LENS and b in R.LENS


def test_case_table_matches_the_issue_and_the_rule():
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)
    for c in R.CASES:
        rule = R.qt_rule(c.B, c.heads, c.T, c.hd)
        assert c.qt == (rule if c.knob == 0 else 3 - rule), c.name
        assert c.hd in (16, 32, 64) or (c.hd == 128 and c.qt == 1 and c.knob == 0), c.name     # (128 x QT 2: an A/B-only instance)
        assert c.heads % c.group == 0 and c.width % 8 == 0 and (c.heads * c.hd) % 4 == 0
        assert c.T * c.width * 2 < 2 ** 31
    packed = [c for c in R.CASES if c.form == "packed"]
    assert {(c.hd, c.qt, c.trim) for c in packed} == {(h, q, t) for h in (16, 32, 64) for q in (1, 2) for t in (0, 1)}
    assert all(c.lens == R.LENS and c.T == 514 and c.B == 21 and c.knob == 0 for c in packed)       # QT from the shape
    assert R.qt_rule(21, 4, 514, 64) == 1 and R.qt_rule(21, 5, 514, 64) == 2
    padded = [c for c in R.CASES if c.form == "padded"]
    assert {(c.hd, c.qt, c.T) for c in padded} == {(h, q, t) for h in (16, 64) for q in (1, 2) for t in (130, 514)}
    assert all(c.B == 5 and min(c.lens) == 1 and max(c.lens) == c.T for c in padded)
    dec = {(c.B, c.T, c.heads, c.group, c.hd, c.qt) for c in R.CASES if c.form == "decoder"}
    assert dec == {(3, 257, 8, 4, 128, 1), (8, 130, 32, 4, 64, 2), (8, 130, 32, 2, 16, 2), (2, 130, 4, 1, 32, 1), (2, 130, 4, 1, 32, 2)}
    ks = set()
    for c in R.CASES:
        if c.form == "decoder":
            ks |= {k if k != c.T - 1 else "T-1" for k in c.kstart}
    assert {0, 1, 63, 64, 65, 100, "T-1"} <= ks
    # the headline encoder shape and the batch-64 OPT-family prefill take the two-tile instances this table covers
    assert R.qt_rule(64, 20, 514, 64) == 2 and R.qt_rule(64, 32, 96, 64) == 2 and R.qt_rule(64, 32, 96, 128) == 1


NAME = "opus_debug_attn_prefill"


def test_signature_is_bound():
    res, args = _cabi.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 26
    assert args[5:13] == [C.c_int64] * 8 and args[-2] == C.POINTER(C.c_int32)
    header = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    assert NAME + "(" in header and "#define OPUS_ABI_VERSION 10" in header
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("so", ["libopus_pllm.so", "libopus_pllm_bf16.so"])
def test_symbol_is_exported(so):
    lib = C.CDLL(os.path.join(ROOT, "opus-pllm_amd", "lib", so))
    assert getattr(lib, NAME) is not None and getattr(lib, "opus_debug_attention") is not None
    assert lib.opus_abi_version() == 10


def test_argument_checks_return_before_any_device_call():
    """A null context is refused first, so none of these can reach the device: null pointers give OPUS_EBADARG (-1) and report
    no QT.  With a context that is only a non-null address the shape checks are reached - they too come before the first device
    call (which would need the context's device): OPUS_ESHAPE (-2), causal with cu OPUS_EUNSUPPORTED (-5)."""
    lib = _cabi.lib()
    qt = C.c_int32(7)
    one = C.c_int64(0)
    p = C.addressof(one)

    def call(ctx=None, Q=p, K=p, V=p, O=p, st=(48, 48, 48, 16), cu=None, B=1, T=16, heads=1, group=1, hd=16, causal=0, trim=0, qtp=None):
        return lib.opus_debug_attn_prefill(ctx, Q, K, V, O, st[0], st[1], st[2], st[3], 0, 0, 0, 0, None, None, cu, B, T, heads, group,
                                           hd, causal, trim, 1.0, C.byref(qt) if qtp is None else qtp, None)

    assert call() == -1 and qt.value == 0 and b"null" in lib.opus_last_error()
    fake = C.c_int64(0)
    ctx = C.addressof(fake)                        # never dereferenced: every call below fails an earlier check
    for kw in (dict(Q=None), dict(K=None), dict(V=None), dict(O=None)):
        qt.value = 7
        assert call(ctx=ctx, **kw) == -1 and qt.value == 0
    assert lib.opus_debug_attn_prefill(ctx, p, p, p, p, 48, 48, 48, 16, 0, 0, 0, 0, None, None, None, 1, 16, 1, 1, 16, 0, 0, 1.0, None,
                                       None) == -1
    for kw in (dict(B=0), dict(T=0), dict(heads=0), dict(group=0), dict(heads=3, group=2), dict(hd=0), dict(st=(0, 48, 48, 16)),
               dict(st=(48, 48, 48, -4)), dict(trim=1), dict(trim=1, cu=p, T=2)):
        qt.value = 7
        assert call(ctx=ctx, **kw) == -2 and qt.value == 0, kw
    assert call(ctx=ctx, causal=1, cu=p) == -5 and b"causal" in lib.opus_last_error()
