"""FP8 decoder weights, CPU side: the twin of the quantiser (tests/w8_ref.py) against torch.float8_e4m3fn and the format's rules,
the FP8 panel layout's index function, and the C ABI additions.  No GPU."""
import os
import re

import pytest
import torch

import w8_ref as W8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.float16, torch.bfloat16)


def _row(absmax, dtype, K=64):
    w = torch.zeros(1, K, dtype=dtype)
    w[0, 3] = absmax
    w[0, 7] = -absmax / 2
    return w


def test_code_table_is_torch_float8_e4m3fn():
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    v = W8.e4m3_values()
    assert torch.equal(torch.isnan(t), torch.isnan(v)) and int(torch.isnan(v).sum()) == 2
    ok = ~torch.isnan(v)
    assert torch.equal(t[ok], v[ok]) and float(v[0x7e]) == W8.E4M3_MAX


def test_rne_is_torch_float8_e4m3fn_on_every_fp16_value_in_range():
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x = x[torch.isfinite(x) & (x.abs() <= 448)].float()
    assert torch.equal(W8.rne_e4m3(x), x.to(torch.float8_e4m3fn).view(torch.uint8))


def test_rne_ties_go_to_the_even_mantissa():
    # halfway between 1 + m / 8 and 1 + (m + 1) / 8, and between the subnormals j 2^-9 and (j + 1) 2^-9
    ties = torch.tensor([1.0625, 1.1875, 1.3125, 1.9375, 2.0 ** -10, 3 * 2.0 ** -10, 15 * 2.0 ** -10, 464.0 / 2, -1.0625, -3 * 2.0 ** -10])
    want = torch.tensor([1.0, 1.25, 1.25, 2.0, 0.0, 2 * 2.0 ** -9, 2.0 ** -6, 224.0, -1.0, -2 * 2.0 ** -9]).double()
    q = W8.rne_e4m3(ties)
    assert torch.equal(W8.e4m3_values()[q.long()], want)
    assert torch.equal(q, ties.to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exponent_rule(dtype):
    above = 1.7578125 if dtype == torch.float16 else 1.765625       # the next operand-type value above 1.75
    lo, hi = W8.LIMITS[dtype]
    cases = [(1.75, -8), (1.75 * 2.0 ** 5, -3), (above, -7), (above * 2.0 ** -4, -11), (1.0, -8), (448.0, 0), (449.0 if dtype == torch.float16 else 450.0, 1),
             (2.0 ** lo, max(lo - 8, W8.EXP_MIN)), (0.0, 0)]
    if dtype == torch.float16:
        cases += [(65504.0, 8), (2.0 ** -24, -32)]
    for absmax, want in cases:
        e = int(W8.row_exponents(_row(absmax, dtype))[0])
        assert e == want, (absmax, e, want)
        if absmax > 0 and want > W8.EXP_MIN:                       # the smallest such integer
            assert absmax * 2.0 ** -e <= 448.0 < absmax * 2.0 ** -(e - 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_matches_float8_and_dq_is_exact(dtype):
    g = torch.Generator().manual_seed(1)
    Wt = torch.cat([(torch.randn(40, 192, generator=g) * torch.logspace(-4, 3, 40)[:, None]).to(dtype), W8.edge_rows(192, dtype)])
    q, e, dq = W8.quantize(Wt)
    assert not ((q & 0x7f) == 0x7f).any()                                       # never NaN
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())[:, None]
    ref = (Wt.double() / scale).float().to(torch.float8_e4m3fn).view(torch.uint8)
    lo, hi = W8.LIMITS[dtype]
    v = W8.e4m3_values()
    refdq = v[ref.long()] * scale
    special = (refdq.abs() < 2.0 ** lo) | (refdq.abs() >= 2.0 ** (hi + 1))       # the subnormal rule / the carry past the largest finite value
    assert torch.equal(q[~special], ref[~special])
    assert (q[refdq.abs() < 2.0 ** lo] == 0).all()                             # +0, not -0
    over = refdq.abs() >= 2.0 ** (hi + 1)
    assert torch.equal(q[over], ref[over] - 1)
    assert torch.equal(dq.double(), v[q.long()] * scale) and torch.isfinite(dq).all()
    assert torch.equal(dq.half().double() if dtype == torch.float16 else dq.bfloat16().double(), dq.double())
    nz = dq != 0
    assert (dq[nz].abs().double() >= 2.0 ** lo).all()                           # every non-zero dq is a normal number
    if dtype == torch.float16:
        assert bool(over.any()) and bool((refdq.abs() < 2.0 ** lo).any())      # the planted rows reach both rules


def test_dq_of_fp16_quantisation_survives_half_and_bfloat16():
    g = torch.Generator().manual_seed(2)
    Wt = (torch.randn(64, 128, generator=g) * 0.02).half()
    _, e, dq = W8.quantize(Wt)
    assert torch.equal(dq.float().half().float(), dq.float()) and torch.equal(dq.float().bfloat16().float(), dq.float())
    rel = ((dq.double() - Wt.double()).pow(2).sum(1) / Wt.double().pow(2).sum(1)).sqrt()
    assert 0.015 < float(rel.mean()) < 0.04                                     # ~2.6 % relative rms on Gaussian rows


def test_nonfinite_weight_is_refused():
    Wt = torch.zeros(16, 64, dtype=torch.float16)
    Wt[3, 5] = float("inf")
    with pytest.raises(ValueError):
        W8.quantize(Wt)


def test_bit_conversion_of_all_254_codes():
    codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
    assert len(codes) == 254
    h = W8.bits_to_half(codes)
    assert torch.equal(h.double() * 256.0, W8.e4m3_values()[codes.long()])


@pytest.mark.parametrize("N,K", [(16, 64), (48, 192), (32, 1088)])
def test_layout_index_and_inverse(N, K):
    seen = set()
    for n in range(N):
        for k in range(K):
            off = W8.tiled_off(n, k, K)
            assert 0 <= off < N * K and W8.tiled_inv(off, K) == (n, k)
            seen.add(off)
    assert len(seen) == N * K
    q = torch.arange(N * K, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(N, K)
    t = W8.tile(q)
    assert torch.equal(W8.untile(t), q)
    flat = t.reshape(-1)
    for n, k in ((0, 0), (5, 37), (N - 1, K - 1), (N - 16, 63)):
        assert flat[W8.tiled_off(n, k, K)] == q[n, k]
    # one lane's 16 bytes: both k-steps of the chunk for one row
    n, c, g = 3, 0, 2
    lane_bytes = flat[(g * 16 + n) * 16:(g * 16 + n) * 16 + 16]
    assert torch.equal(lane_bytes[:8], q[n, 64 * c + 8 * g:64 * c + 8 * g + 8]) and torch.equal(lane_bytes[8:], q[n, 64 * c + 32 + 8 * g:64 * c + 40 + 8 * g])


def test_header_has_the_new_symbols_at_abi_10():
    h = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    assert re.search(r"#define OPUS_ABI_VERSION 10\b", h)
    for sym in ("opus_quantize_fp8", "opus_debug_gemm_w8", "OPUS_F8E4M3 = 5", "OPUS_I8 = 6"):
        assert sym in h, sym
    from opus_pllm_amd import _cabi
    assert _cabi.ABI_VERSION == 10 and "opus_quantize_fp8" in _cabi.SIGNATURES and "opus_debug_gemm_w8" in _cabi.SIGNATURES
    assert (_cabi.OPUS_F8E4M3, _cabi.OPUS_I8) == (5, 6)


def test_keyword_is_validated_and_load_4bit_is_untouched():
    import inspect
    from opus_pllm_amd import builder, weights
    assert weights.DECODER_WEIGHT_FORMATS == (None, "fp8", "fp8_dequantized", "mxfp4", "mxfp4_dequantized")
    for fn in (weights.DeviceWeights.from_canonical, weights.DeviceWeights.synthetic):
        assert inspect.signature(fn).parameters["decoder_weights"].default is None
    src = inspect.getsource(builder.load_pretrained_model)
    assert "decoder_weights" in src and "loading unquantised fp16" in src
    import opus_pllm_amd as opa
    assert weights.quantized_names(opa.micro())[:4] == ["dec.0.wqkv", "dec.0.wo", "dec.0.wgu", "dec.0.wd"]
