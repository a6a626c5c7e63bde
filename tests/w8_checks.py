"""One case of tests/gemm_cells_ref.py with the FP8 form of W offered beside it (opus_debug_gemm_w8), on the poisoned layout of
tests/gemm_cells_checks.run_case plus the FP8 poison: shared by tests/test_gpu_w8.py and the bf16 child tests/bf16_w8_check.py.
Not product code.

Poisoned layout: A is the first M rows of a buffer whose following rows are NaN; the padded rows N .. Npad - 1 of the fp16 copy of
W are NaN and the same rows of the FP8 panels hold the NaN code 0x7f, as do 4 KB behind the panels; the row exponents behind row
N - 1 are 127 (2^127: a use would show); the output has GUARD_ROWS sentinel rows behind row M - 1.
"""
from __future__ import annotations

import ctypes as C

import torch

import gemm_cells_checks as K
import gemm_cells_ref as R
import w8_ref as W8
from opus_pllm_amd import _cabi
from opus_pllm_amd.weights import quantize_fp8, tile_weight

W8_CLASSES = (R.SKINNY, R.MID, R.WIDE, R.STREAM)   # the weight-streaming classes: each has an FP8 instantiation; ring / tile / pp read the fp16 copy


def fp8_operand(W, N):
    """W [N, K] operand type on the GPU -> (dW: panel-tiled dq with NaN pad rows, q8 poisoned FP8 panels, e8 poisoned, dq [N, K])"""
    dev, Npad, Kk = W.device, R.cdiv(N, 16) * 16, W.shape[1]
    Wp = torch.zeros((Npad, Kk), dtype=W.dtype, device=dev)
    Wp[:N] = W
    q8, e8, dq = quantize_fp8(Wp)
    rows = W8.untile(q8)
    rows[N:] = 0x7f
    buf = torch.full((Npad * Kk + 4096,), 0x7f, dtype=torch.uint8, device=dev)
    buf[:Npad * Kk] = W8.tile(rows).reshape(-1)
    ebuf = torch.full((Npad + 64,), 127, dtype=torch.int8, device=dev)
    ebuf[:N] = e8[:N]
    dqp = torch.full((Npad, Kk), float("nan"), dtype=W.dtype, device=dev)
    dqp[:N] = dq[:N]
    return tile_weight(dqp), buf, ebuf, dq[:N]


def launch(ctx, form, A, dW, q8, e8, bias, res_out, out, c, eps=1e-5):
    ks, ran = C.c_int32(-1), C.c_int32(-1)
    _cabi.check(_cabi.lib().opus_debug_gemm_w8(
        ctx, form, A.data_ptr(), dW.data_ptr(), q8.data_ptr(), e8.data_ptr(), None if bias is None else bias.data_ptr(),
        None if res_out is None else res_out.data_ptr(), out.data_ptr(), c.M, c.N, c.K, 0 if form == 2 else c.epi,
        1 if c.mode != R.F16 else 0, eps, C.byref(ks), C.byref(ran), None))
    return ks.value, ran.value


def run_exact_case(ctx, dev, c, repeats=1):
    """The exact input family through opus_debug_gemm_w8.  With the norm fused the activations are the exact family's integers as
    fp32 (the norm itself is not exact: held to fp64 within NORM_RULE)."""
    dt = _cabi.operand_dtype()
    nout = c.N // 2 if c.epi == R.SILU else c.N
    out_dt = torch.float32 if c.mode != R.F16 else dt
    Ai, Wi, bi, ri, e = R.exact_inputs(c)
    Ai, Wi, bi = Ai.to(dev), Wi.to(dev), bi.to(dev)
    ri = None if ri is None else ri.to(dev)
    W = (Wi.float() * 2.0 ** -e).to(dt)
    dW, q8, e8, dq = fp8_operand(W, c.N)
    obs = {"id": R.case_id(c), "quantiser_reproduces_w": bool(torch.equal(dq, W))}
    if c.norm:
        A = K._poisoned(Ai.float(), R.a_rows(c.M))
        bias, res = None, None
        pre, ref = None, R.norm_reference(Ai.float(), W, c.epi)
    else:
        A = K._poisoned(Ai.to(dt), R.a_rows(c.M))
        bias = None if c.slab else bi.float() * 2.0 ** -e
        res = None if ri is None else ri.float() * 2.0 ** -e
        pre, ref = R.exact_reference(Ai, Wi, torch.zeros_like(bi) if c.slab else bi, ri, e, R.PLAIN if c.slab else c.epi)
    if c.a_tiled:
        A = tile_weight(A)
    A0, W0, q0, e0 = A.clone(), dW.clone(), q8.clone(), e8.clone()
    outs, plans, rans = [], [], []
    lib = _cabi.lib()
    if c.a_tiled:
        _cabi.check(lib.opus_debug_knob(ctx, b"debug_a_tiled", 1))
    try:
        for _ in range(repeats):
            if c.slab:
                out = torch.full((8 * c.M * c.N + R.GUARD_ROWS * c.N,), R.SENTINEL, dtype=torch.float32, device=dev)
                ks, ran = launch(ctx, 2, A, dW, q8, e8, None, None, out, c)
                obs["ks"] = ks
            else:
                out = torch.full((c.M + R.GUARD_ROWS, nout), R.SENTINEL, dtype=out_dt, device=dev)
                if res is not None:
                    out[:c.M] = res
                ks, ran = launch(ctx, 1 if c.norm else 0, A, dW, q8, e8, bias, out if res is not None else None, out, c)
            plans.append(K.report(ctx))
            rans.append(ran)
            outs.append(out)
        torch.cuda.synchronize()
    finally:
        if c.a_tiled:
            _cabi.check(lib.opus_debug_knob(ctx, b"debug_a_tiled", 0))
    obs["plans"] = [list(p) for p in plans]
    obs["ran_w8"] = rans
    obs["repeats_equal"] = all(torch.equal(K._bits(outs[0]), K._bits(o)) for o in outs[1:])
    obs["bystanders_untouched"] = bool(torch.equal(K._bits(A), K._bits(A0)) and torch.equal(K._bits(dW), K._bits(W0)) and
                                       torch.equal(q8, q0) and torch.equal(e8, e0))
    out = outs[0]
    if c.slab:
        ks = max(obs["ks"], 1)
        used = ks * c.M * c.N
        obs["guard_untouched"] = bool((out[used:] == R.SENTINEL).all())
        slabs = out[:used].view(ks, c.M, c.N)
        obs["finite"] = bool(torch.isfinite(slabs).all())
        obs["exact"] = bool(torch.equal(slabs.double().sum(0), pre))
        return obs
    obs["guard_untouched"] = bool((out[c.M:] == R.SENTINEL).all())
    got = out[:c.M]
    obs["finite"] = bool(torch.isfinite(got).all())
    if not c.norm and c.epi == R.PLAIN:
        want = ref.to(out_dt)
        obs["exact"] = bool(torch.equal(got, want))
        obs["n_diff"] = int((got != want).sum())
    obs["err"] = float((got.double() - ref).abs().max())
    obs["ref_max"] = float(ref.abs().max())
    return obs


def failures(c, obs, bf16=False):
    """K.failures (route == the case's plan, poison, exactness / the kernel rules) + the FP8 assertions."""
    bad = K.failures(c, obs, bf16)
    if not obs["quantiser_reproduces_w"]:
        bad.append("the quantiser did not reproduce the e4m3-exact weights")
    want = 1 if c.plan.klass in W8_CLASSES else 0
    if any(r != want for r in obs["ran_w8"]):
        bad.append(f"ran_w8 {obs['ran_w8']}, expected {want}")
    return bad


# ------------------------------------------------------------------------------------------------ Gaussian operands
def row_exponent_spread(N):
    """Per-row scale exponents 7 .. -7: they differ by 7 inside a 16-row panel and by 7 between the members of a gate / up pair
    (rows n and n + 16 of a 32-row group), give or take one for the rows' own absmax: a mixed-up exponent index cannot hide.
    (The range keeps every weight a normal fp16 number and silu(g) u inside fp16.)"""
    n = torch.arange(N)
    return (7 - (n % 8) - 7 * ((n // 16) % 2)).double()


def run_gaussian_case(ctx, dev, c):
    """gaussian_inputs with the rows of W spread over 15 binades; reference: fp64 on (the operand-type A, dq)."""
    dt = _cabi.operand_dtype()
    nout = c.N // 2 if c.epi == R.SILU else c.N
    X, Wg = R.gaussian_inputs(c)
    Wg = (Wg.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), row_exponent_spread(c.N))[:, None]).to(dt).to(dev)
    dW, q8, e8, dq = fp8_operand(Wg, c.N)
    e_rows = e8[:c.N].int()
    obs = {"id": R.case_id(c), "exp_spread_in_panel": int((e_rows[:16].max() - e_rows[:16].min())),
           "dq_rel_rms": float(((dq.double() - Wg.double()).norm() / Wg.double().norm()))}
    if c.epi == R.SILU:
        obs["exp_spread_in_pair"] = int((e_rows[:16] - e_rows[16:32]).abs().min())
    out_dt = torch.float32 if c.mode != R.F16 else dt
    out = torch.full((c.M + R.GUARD_ROWS, nout), R.SENTINEL, dtype=out_dt, device=dev)
    if c.norm:
        A = K._poisoned(X.to(dev), R.a_rows(c.M))
        ref = R.norm_reference(X.to(dev), dq, c.epi)
        _, ran = launch(ctx, 1, A, dW, q8, e8, None, None, out, c)
    else:
        A16 = X.to(dt).to(dev)
        A = K._poisoned(A16, R.a_rows(c.M))
        ref = R.activate(A16.double() @ dq.double().T, c.epi)
        if c.a_tiled:
            A = tile_weight(A)
            _cabi.check(_cabi.lib().opus_debug_knob(ctx, b"debug_a_tiled", 1))
        try:
            _, ran = launch(ctx, 0, A, dW, q8, e8, None, None, out, c)
        finally:
            if c.a_tiled:
                _cabi.check(_cabi.lib().opus_debug_knob(ctx, b"debug_a_tiled", 0))
    torch.cuda.synchronize()
    obs["plans"] = [list(K.report(ctx))]
    obs["ran_w8"] = [ran]
    obs["guard_untouched"] = bool((out[c.M:] == R.SENTINEL).all())
    got = out[:c.M]
    obs["finite"] = bool(torch.isfinite(got).all())
    obs["err"] = float((got.double() - ref).abs().max())
    obs["ref_max"] = float(ref.abs().max())
    obs["bystanders_untouched"] = obs["repeats_equal"] = True
    return obs
