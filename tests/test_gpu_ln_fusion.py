"""The LayerNorm (encoder) and RMSNorm (decoder prefill) fused around gemm_pp_kernel, against fp64, on every launch path.

The norm is split over three places: the GEMM that writes the residual stream also writes fp16(x) and per-64-column
(sum x, sum x^2) partials; ln_finalize_kernel turns them into (mu, rstd); the next projection runs on the un-normalised fp16(x) and
applies rstd (acc - mu s) + c2 in its epilogue.  That arithmetic exists in the main epilogue, in the in-launch pair combine and in
pp_tail_reduce_kernel, on the producer and on the consumer side, and launch_pp picks among them from the tile count modulo 256,
K and the workspace.  opus_debug_gemm_ln runs the chain as the path issues it and reports launch_pp's plan for both GEMMs; every
case below ASSERTS the plan it was chosen for (tests/ln_fusion_checks.py holds the per-stage checks and the row statistics, which
tests/ln_fusion_ref.py defines; tests/test_ln_fusion_host.py checks that reference on the CPU).

Cells.  Producer (EPI_NONE, fp32 output + residual): {no tail, pair, reduce with 3 - 8 parts} x {ragged last row tile,
M % 256 == 0}, N1 in {1280, 2560, 4096, 5120} (20 / 40 / 64 / 80 slabs in ln_finalize), M % 16 != 0 in the ragged cases.
Consumer: LayerNorm + bias, LayerNorm + GELU, RMSNorm, RMSNorm + gate / up, each x {no tail, pair, reduce}; LayerNorm + fused rotary
with row % T positions and with a position table - without a tail split, which the rotary switches off (launch_pp: the rotation
runs in gemm_pp_kernel's own epilogue only).  No legal cell turned out unreachable.

Per stage (whole matrices, so every tail tile and the whole last row tile are covered):
  X            fp64, the project's rule for a GEMM output (2e-3 max |ref| + 1e-5), per class of rows
  fp16(X)      == X rounded, bit for bit
  partials     fp64 sums of the X the kernel wrote; error measured against sum |x| (sum x^2) of the slab; bound 4 x the worst error
               of the fp32 emulation in the kernel's summation order on the same data (observed emulation worst 1.5e-7 .. 1.8e-7:
               bounds 6e-7 .. 7e-7) - the factor covers the fused multiply-adds the compiler may or may not form
  (mu, rstd)   fp64 of the same X; bound per class 4 x (the emulation's worst error there over the contraction variants + 1 ulp
               for rsqrtf): ~1e-6 at mu / sigma = 0, ~5e-5 at 8, 3e-3 .. 4e-3 at 64 - it grows as 1 + mu^2 / var, as E[x^2] - mu^2 does
  consumer     the kernel's own algebra in fp64 on the fp16(X) and (mu, rstd) the DEVICE produced: 2e-3 max |ref| + 1e-5 (3e-3
               max |ref| behind the rotary, as test_fused_rotary_epilogue_is_the_standalone_kernel) - whatever the statistics,
               this fails on an indexing, combine or launcher bug
  accuracy     exact norm then GEMM in fp64, per class: the host model's fused-form error on those rows + the kernel rule;
               the fused and the stand-alone form's measured errors are record()ed side by side
Nothing behind row M of any buffer may be written (sentinels).  Values beyond the fp16 range are out of scope for the fp16
build: the un-normalised fp16(x) hand-off cannot represent them.
"""
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
from gpu_helpers import record
from ln_fusion_checks import NONE, PAIR, REDUCE, check_case, make_ctx, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wide_ctx(dev):
    """A full-width context (Llama-3-8B + ESM2-650M shapes, batch 64) without weights: the chain needs the GEMM workspace, the
    hand-off words and the encoder's rotary table only."""
    cfg = opa.llama3_8b(max_batch=64, max_enc_tokens=1026, max_prompt=104, max_new_tokens=16)
    ctx = make_ctx(cfg, dev)
    _cabi.check(_cabi.lib().opus_check_error(ctx, None))
    yield cfg, ctx
    _cabi.check(_cabi.lib().opus_check_error(ctx, None))       # no hand-off of the module gave up waiting
    _cabi.lib().opus_ctx_destroy(ctx)
    torch.cuda.empty_cache()


LN, RMS = False, True
# (id, M, N1, K1, N2, epi, rms, rope, producer bias, producer tail, its k-parts, consumer tail).  With T = ceil(M / 256) N / 256
# tiles and R = T mod 256, launch_pp cuts the last R tiles (T > 256, R <= 128) into sp = min(256 / R, 8, K / 256) k-parts when
# (1.5 K / 64 + 12)(1 - 1 / sp) exceeds 22 (two parts, combined in the launch) or 30 (slabs + pp_tail_reduce_kernel).
CASES = [
    # ESM2-650M widths: wo (K = 1280) / fc2 (K = 5120) produce, QKV (3840) / fc1 (5120) consume at K = 1280 (never a pair there)
    ("ln_wo_ragged__fc1_gelu_reduce", 10140, 1280, 1280, 5120, 1, LN, None, True, NONE, 1, REDUCE),
    ("ln_wo_even__qkv_reduce", 9216, 1280, 1280, 3840, 0, LN, None, False, NONE, 1, REDUCE),
    ("ln_fc2_pair_ragged__qkv_rope_row", 18355, 1280, 5120, 3840, 0, LN, "row", False, PAIR, 2, NONE),
    ("ln_fc2_pair_even__fc1_gelu", 18432, 1280, 5120, 5120, 1, LN, None, False, PAIR, 2, NONE),
    ("ln_fc2_reduce8_ragged__qkv_rope_pos", 14329, 1280, 5120, 3840, 0, LN, "pos", False, REDUCE, 8, NONE),
    ("ln_fc2_reduce8_even__qkv", 14336, 1280, 5120, 3840, 0, LN, None, True, REDUCE, 8, NONE),
    # ESM2-3B widths (K = 2560: long enough for a pair on the consumer side)
    ("ln3b_pair_even__fc1_gelu_pair", 8960, 2560, 2560, 10240, 1, LN, None, False, PAIR, 2, PAIR),
    ("ln3b_reduce7_ragged__qkv_pair", 7411, 2560, 2560, 7680, 0, LN, None, False, REDUCE, 7, PAIR),
    # Llama-3-8B prefill: wo (K = 4096) / down (K = 14336) produce, QKV (6144) / gate-up (28672) consume
    ("rms_wo_pair_ragged__qkv_reduce", 5619, 4096, 4096, 6144, 0, RMS, None, False, PAIR, 2, REDUCE),
    ("rms_wo_reduce8_even__gateup_pair", 4352, 4096, 4096, 28672, 2, RMS, None, False, REDUCE, 8, PAIR),
    ("rms_wo_reduce5_ragged__gateup_reduce", 4853, 4096, 4096, 28672, 2, RMS, None, False, REDUCE, 5, REDUCE),
    ("rms_wo_even__qkv_pair", 4096, 4096, 4096, 6144, 0, RMS, None, False, NONE, 1, PAIR),
    ("rms_down_reduce8_ragged__qkv", 4603, 4096, 14336, 6144, 0, RMS, None, False, REDUCE, 8, NONE),
    ("rms_wo_ragged__gateup", 4090, 4096, 4096, 28672, 2, RMS, None, False, NONE, 1, NONE),
    # Vicuna-13B prefill widths (80 slabs: two rounds of ln_finalize's loop)
    ("rms13b_pair_even__qkv_reduce", 4608, 5120, 5120, 15360, 0, RMS, None, False, PAIR, 2, REDUCE),
    ("rms13b_reduce8_ragged__gateup", 3575, 5120, 5120, 27648, 2, RMS, None, False, REDUCE, 8, NONE),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_norm_chain_vs_fp64(wide_ctx, dev, case):
    name, M, N1, K1, N2, epi, rms, rope, b1, want_p, parts, want_c = case
    cfg, ctx = wide_ctx
    assert (M % 256 == 0) == ("even" in name.split("__")[0]) and (M % 256 == 0 or M % 16 != 0)
    res = run_case(ctx, dev, M, N1, K1, N2, epi=epi, rms=rms, rope=rope, b1=b1, seed=len(name), rope_theta=cfg.enc_rope_theta)
    print("ln_fusion", name, "producer plan", res["plan_producer"], "consumer plan", res["plan_consumer"])
    record("ln_fusion." + name, res)
    check_case(res, want_p, want_c, parts)


def test_pair_combine_repeats_bit_identically(wide_ctx, dev):
    """Two-part tail tiles are combined by whichever half arrives second (producer: fc2 at 360 tiles; consumer: fc1 of the 3B
    widths): six more runs of the same chain give the same bits in X, fp16(X), the partials, (mu, rstd) and the output, as
    test_pingpong_gemm_repeats_bit_identically asks of the plain epilogues."""
    cfg, ctx = wide_ctx
    res = run_case(ctx, dev, 8960, 2560, 2560, 10240, epi=1, seed=3, repeats=6, standalone=False)
    print("ln_fusion pair_repeats producer plan", res["plan_producer"], "consumer plan", res["plan_consumer"])
    check_case(res, PAIR, PAIR, 2)
    res = run_case(ctx, dev, 18432, 1280, 5120, 5120, epi=1, seed=4, repeats=6, standalone=False)
    check_case(res, PAIR, NONE, 2)


def test_shape_off_the_fused_form_is_reported_not_replaced(wide_ctx, dev):
    """Too few tiles for gemm_pp_kernel: the producer GEMM runs on another kernel, leaves no partials, and the entry says so
    (*produced = 0, plan untouched) instead of normalising some other way."""
    cfg, ctx = wide_ctx
    res = run_case(ctx, dev, 1000, 1280, 1280, 3840)
    assert res["produced"] == 0 and res["plan_producer"] == [-1] * 5 and res["plan_consumer"] == [-1] * 5, res
