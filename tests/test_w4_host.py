"""MXFP4 decoder weights, CPU side: the twin of the quantiser (tests/w4_ref.py) against a brute-force fp64 search and the format's
rules, the code / scale panel layout's index functions, and the C ABI additions.  No GPU."""
import os
import re

import pytest
import torch

import w4_ref as W4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.float16, torch.bfloat16)
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0)


def _brute(v: torch.Tensor) -> torch.Tensor:
    """nearest of the 8 magnitudes to min(v, 6) in fp64, ties to the even code - the independent formulation"""
    vals = torch.tensor(W4.VALUES, dtype=torch.float64)
    d = (v.double().clamp(max=6.0)[:, None] - vals[None, :]).abs()
    best = d.min(dim=1).values
    out = torch.empty(len(v), dtype=torch.int64)
    for i in range(len(v)):
        c = [j for j in range(8) if d[i, j] == best[i]]
        assert len(c) in (1, 2)
        out[i] = c[0] if len(c) == 1 else next(j for j in c if j % 2 == 0)
    return out


def test_rne_is_the_brute_force_search_on_every_fp16_value_below_8():
    x = torch.arange(32768, dtype=torch.int32).to(torch.int16).view(torch.float16)           # every non-negative fp16
    x = torch.cat([x[x < 8].float(), torch.tensor(TIES)])
    got = W4.rne_e2m1(x.view(torch.int32).long())
    assert torch.equal(got, _brute(x))
    ties = W4.rne_e2m1(torch.tensor(TIES).view(torch.int32).long())
    assert [W4.VALUES[int(c)] for c in ties] == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0]        # the even code; 7 saturates


def test_quantize_is_the_brute_force_search_on_one_scaled_block():
    # every fp16 value in [0, 8) as one block's members (absmax 7.99..: e = 0), both signs, plus the planted ties
    x = torch.arange(32768, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x = x[x < 8]
    x = torch.cat([x, torch.tensor(TIES, dtype=torch.float16), -x])
    pad = (-len(x)) % 32
    x = torch.cat([x, torch.zeros(pad, dtype=torch.float16)])
    top = x.abs().max()
    W = x.reshape(-1, 32).clone()
    W[:, 31] = top                                                     # the same absmax, hence e = 0, in every block
    q, s, dq = W4.quantize(W.reshape(1, -1))
    assert (s == 127).all()
    want = _brute(W.reshape(-1).float().abs())
    assert torch.equal((q.reshape(-1) & 7).long(), want)
    neg = (W.reshape(-1) < 0) & (want > 0)
    assert torch.equal((q.reshape(-1) >> 3).bool(), neg)
    assert torch.equal(dq.double(), W4.dequantize(q, s))


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_rule_and_edge_blocks(dtype):
    lo, hi = W4.LIMITS[dtype]

    def block(absmax, small=None):
        w = torch.zeros(1, 64, dtype=dtype)
        w[0, 3] = absmax
        if small is not None:
            w[0, 9] = small
        return w

    for mant in (1.0, 1.4921875, 1.5, 1.9921875):
        for x in (-9, 0, 6):
            q, s, dq = W4.quantize(block(mant * 2.0 ** x))
            e = int(s[0, 0]) - 127
            assert e == x - 2 and int(s[0, 1]) == 127                 # floor(log2) - 2; the all-zero block: e = 0
            # 4 <= absmax 2^-e < 8: mantissa 1.0 -> 4, 1.49 -> 6 (5.97 is above the tie at 5), 1.5 -> 6, 1.99 -> 6 (saturated)
            assert float(dq[0, 3]) == (4.0 if mant == 1.0 else 6.0) * 2.0 ** e
    # the smallest normal: e = lo - 2, q = 4 -> dq = absmax; 2^e itself is below the normal range, so codes below 4 x ... flush
    # (bf16: lo - 2 = -128 is below the floor of the exponents, e = EXP_MIN and 2^lo 2^-e = 2^-6 rounds to 0 - weights below
    #  2^-122 are out of the format's reach, as in the FP8 form)
    q, s, dq = W4.quantize(block(2.0 ** lo, 2.0 ** (lo - 1)))
    assert int(s[0, 0]) - 127 == max(lo - 2, W4.EXP_MIN) and float(dq[0, 3]) == (2.0 ** lo if dtype == torch.float16 else 0.0)
    assert float(dq[0, 9]) == 0.0 and int(q[0, 9]) == 0               # 2 x 2^e = 2^(lo-1) would be subnormal: +0
    # one below the smallest normal (the largest subnormal): everything in the block flushes
    sub = torch.tensor(2.0 ** lo).to(dtype).view(torch.int16) - 1
    q, s, dq = W4.quantize(block(float(sub.view(dtype))))
    assert (q == 0).all() and (dq == 0).all()
    if dtype == torch.float16:
        assert int(s[0, 0]) - 127 == lo - 3
    # the largest finite value stays finite: q = 6 at e = hi - 2
    big = float(torch.tensor(torch.finfo(dtype).max))
    q, s, dq = W4.quantize(block(big, -big))
    assert int(s[0, 0]) - 127 == hi - 2 and float(dq[0, 3]) == 6.0 * 2.0 ** (hi - 2) and torch.isfinite(dq).all()
    assert int(q[0, 3]) == 7 and int(q[0, 9]) == 15
    assert 1 <= int(s.min()) and int(s.max()) <= 254
    # an all-zero block and negative zeros: +0 codes, scale byte 127
    w = torch.zeros(1, 64, dtype=dtype)
    w[0, 5] = -0.0
    q, s, dq = W4.quantize(w)
    assert (q == 0).all() and (s == 127).all() and (dq.view(torch.int16) == 0).all()
    # a negative value that rounds to zero is +0 too
    q, s, dq = W4.quantize(block(4.0, -0.2))
    assert int(q[0, 9]) == 0 and dq.view(torch.int16)[0, 9] == 0
    if dtype == torch.bfloat16:                                        # the floor of the block exponents
        q, s, dq = W4.quantize(block(2.0 ** -125))
        assert int(s[0, 0]) - 127 == W4.EXP_MIN and float(dq[0, 3]) == 0.0
        assert float(W4.quantize(block(2.0 ** -119))[2][0, 3]) == 2.0 ** -119


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_rows_quantise_exactly_and_reach_the_rules(dtype):
    lo, hi = W4.LIMITS[dtype]
    Wt = W4.edge_rows(192, dtype)
    q, s, dq = W4.quantize(Wt)
    assert torch.equal(dq.double(), W4.dequantize(q, s)) and torch.isfinite(dq).all()
    assert not (q == 8).any()                                          # never a negative zero
    nz = dq != 0
    assert (dq[nz].abs().double() >= 2.0 ** lo).all()                  # every non-zero dq is a normal number
    scaled = Wt.double().abs() / torch.pow(torch.tensor(2.0, dtype=torch.float64), s.double() - 127).repeat_interleave(32, dim=1)
    assert bool(((scaled > 6) & (scaled < 8)).any())                   # saturation is reached
    want = _brute(scaled.reshape(-1)).reshape(scaled.shape)
    kept = nz | (want == 0)
    assert torch.equal((q & 7).long()[kept], want[kept])               # the brute-force search wherever the flush rule did not act
    flushed = ~kept
    # the flush rule is reached in fp16 (in bf16 the floor of the exponents, 2^-120, keeps every non-zero code a normal number)
    assert bool(flushed.any()) == (dtype == torch.float16)
    assert (W4.dequantize(want.to(torch.uint8), s)[flushed].abs() < 2.0 ** lo).all()


def test_dq_is_exact_in_half_and_bfloat16_and_the_error_is_the_expected_one():
    g = torch.Generator().manual_seed(2)
    W32 = torch.randn(256, 4096, generator=g) * 0.02
    for dtype in DTYPES:
        Wt = W32.to(dtype)
        _, _, dq = W4.quantize(Wt)
        assert torch.equal(dq.float().half().float(), dq.float()) and torch.equal(dq.float().bfloat16().float(), dq.float())
        rel = ((dq.double() - Wt.double()).pow(2).sum(1) / Wt.double().pow(2).sum(1)).sqrt()
        print("mxfp4 mean per-row relative rms error", dtype, float(rel.mean()))
        assert 0.10 < float(rel.mean()) < 0.13                         # ~11.4 % on Gaussian rows


def test_nonfinite_weight_is_refused():
    Wt = torch.zeros(16, 64, dtype=torch.float16)
    Wt[3, 5] = float("inf")
    with pytest.raises(ValueError):
        W4.quantize(Wt)


@pytest.mark.parametrize("N,K", [(16, 64), (48, 192), (32, 1088)])
def test_layout_index_and_inverse(N, K):
    seen = set()
    for n in range(N):
        for k in range(K):
            off, nib = W4.tiled_off(n, k, K)
            assert 0 <= off < N * K // 2 and nib == k % 2 and W4.tiled_inv(off, nib, K) == (n, k)
            seen.add((off, nib))
    assert len(seen) == N * K
    sseen = set()
    for n in range(N):
        for kb in range(K // 32):
            off = W4.scale_off(n, kb, K)
            assert 0 <= off < N * K // 32 and W4.scale_inv(off, K) == (n, kb)
            sseen.add(off)
    assert len(sseen) == N * K // 32
    q = torch.arange(N * K, dtype=torch.int64).remainder(13).add(torch.arange(N * K) // 7).remainder(16).to(torch.uint8).reshape(N, K)
    s = torch.arange(N * K // 32, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(N, K // 32)
    t, ts = W4.tile(q), W4.tile_scales(s)
    assert t.shape == (N, K // 2) and torch.equal(W4.untile(t), q) and torch.equal(W4.untile_scales(ts), s)
    flat, sflat = t.reshape(-1), ts.reshape(-1)
    for n, k in ((0, 0), (5, 37), (N - 1, K - 1), (N - 16, 63)):
        off, nib = W4.tiled_off(n, k, K)
        assert (int(flat[off]) >> (4 * nib)) & 15 == int(q[n, k])
        assert int(sflat[W4.scale_off(n, k // 32, K)]) == int(s[n, k // 32])
    # one lane's 8 code bytes: both k-steps of the chunk for one row, the lower k in the low nibble; its 2 scale bytes
    n, c, g = 3, K // 64 - 1, 2
    base = ((n // 16) * (K // 64) + c) * 512 + (g * 16 + n % 16) * 8
    lane_bytes = flat[base:base + 8]
    codes = torch.stack((lane_bytes & 15, lane_bytes >> 4), dim=-1).reshape(-1)
    assert torch.equal(codes[:8], q[n, 64 * c + 8 * g:64 * c + 8 * g + 8]) and torch.equal(codes[8:], q[n, 64 * c + 32 + 8 * g:64 * c + 40 + 8 * g])
    sbase = ((n // 16) * (K // 64) + c) * 32 + (n % 16) * 2
    assert torch.equal(sflat[sbase:sbase + 2], s[n, 2 * c:2 * c + 2])
    # codes plus scales: at most 0.27 of the fp16 tensor's bytes
    assert (t.numel() + ts.numel()) <= 0.27 * 2 * N * K


def test_package_untile_is_the_twins():
    from opus_pllm_amd.weights import untile_mxfp4
    q = torch.arange(48 * 192).remainder(16).to(torch.uint8).reshape(48, 192)
    s = torch.arange(48 * 6).remainder(200).to(torch.uint8).reshape(48, 6)
    cq, cs = untile_mxfp4(W4.tile(q), W4.tile_scales(s))
    assert torch.equal(cq, q) and torch.equal(cs, s)


def test_header_has_the_new_symbols_at_abi_10():
    h = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    assert re.search(r"#define OPUS_ABI_VERSION 10\b", h)
    for sym in ("opus_quantize_mxfp4", "opus_debug_gemm_w4", "OPUS_F4E2M1X2 = 7", "OPUS_E8M0 = 8", "OPUS_I8 = 6", "w4_gemms"):
        assert sym in h, sym
    from opus_pllm_amd import _cabi
    assert _cabi.ABI_VERSION == 10 and "opus_quantize_mxfp4" in _cabi.SIGNATURES and "opus_debug_gemm_w4" in _cabi.SIGNATURES
    assert (_cabi.OPUS_F4E2M1X2, _cabi.OPUS_E8M0) == (7, 8)
    assert _cabi.SIGNATURES["opus_debug_gemm_w4"] == _cabi.SIGNATURES["opus_debug_gemm_w8"]


def test_keywords_are_validated_and_load_4bit_is_untouched():
    import inspect
    import opus_pllm_amd as opa
    from opus_pllm_amd import builder, weights
    assert weights.DECODER_WEIGHT_FORMATS == (None, "fp8", "fp8_dequantized", "mxfp4", "mxfp4_dequantized")
    for fn in (weights.DeviceWeights.from_canonical, weights.DeviceWeights.synthetic):
        assert inspect.signature(fn).parameters["decoder_weights"].default is None
    w = weights.DeviceWeights(opa.micro(), torch.device("cpu"))
    for fmt in weights.DECODER_WEIGHT_FORMATS:
        w._set_decoder_weights(fmt)
        assert w.decoder_weights == fmt
    assert w.decoder_weight_format == "mxfp4_dequantized"
    for bad in ("nf4", "mxfp8", "int4", "MXFP4"):
        with pytest.raises(ValueError):
            w._set_decoder_weights(bad)
    src = inspect.getsource(builder.load_pretrained_model)
    assert "decoder_weights" in src and "loading unquantised fp16" in src and "mxfp4" in src
    for script in ("eval_ddp.py", "eval_multichoice.py", "eval_online.py"):
        assert '"mxfp4"' in open(os.path.join(ROOT, "opus-pllm_amd", script)).read()
