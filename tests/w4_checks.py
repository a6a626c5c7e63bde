"""One case of tests/gemm_cells_ref.py with the MXFP4 form of W offered beside it (opus_debug_gemm_w4), on the poisoned layout of
tests/gemm_cells_checks.run_case plus the MXFP4 poison: shared by tests/test_gpu_w4.py and the bf16 child tests/bf16_w4_check.py.
Not product code.

Poisoned layout: A is the first M rows of a buffer whose following rows are NaN; the padded rows N .. Npad - 1 of the 16-bit copy of
W are NaN and the same rows of the scale panels hold 255 (e8m0's NaN), as do 64 bytes behind the scale panels; 4 KB of 0x77 follow
the code panels; the output has GUARD_ROWS sentinel rows behind row M - 1.

Exact operands.  The exact family of gemm_cells_ref holds integers up to 7, which e2m1 cannot (no 5, no 7), so this file has its
own: W = code value x 2^(base + j), the codes uniform over all 16 (negative zero included: the panels are built by the twin's tile
functions, not by the quantiser), j = (n + 7 kb) % 8 - eight binades inside every 16-row panel AND along K, so every code meets
eight scale bytes in every case.  A = integers -amax .. amax without 0 (amax = 7, 3 when K > 8192) x 2^-ea.  In units of
2^(base - 1 - ea) every product and every partial sum in any order is an integer; the case checks sum |a| |w| < 2^24 on its own
operands (exact_sums), so the fp32 sums are exact and the fp64 matmul of the operands is THE result, to the bit.  base / ea put the
pre-activation's standard deviation at about 1 .. 3 and keep every weight a normal fp16 number (base >= -13).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

import gemm_cells_checks as K
import gemm_cells_ref as R
import w4_ref as W4
import w8_checks as Q
from opus_pllm_amd import _cabi
from opus_pllm_amd.weights import quantize_mxfp4, tile_weight, untile_mxfp4

W4_CLASSES = (R.SKINNY, R.MID, R.WIDE, R.STREAM)   # the weight-streaming classes: each has an MXFP4 instantiation
SPREAD = 8                                         # binades of block scales inside a panel and along K
W_RMS = math.sqrt(8.5625 * 21845.0 / 8.0)          # rms of code value x 2^j: mean of the squared magnitudes x mean of 4^j, j = 0 .. 7


def _dq(q, s, dt):
    """codes [N, K] and scale bytes [N, K / 32] (row-major, on any device) -> the dequantised weights in dt (exact)"""
    two_e = ((s.long() - 127 + 1023) << 52).view(torch.float64)      # 2^(s - 127) from its bits (pow / ldexp on the GPU are not exact)
    v = W4.e2m1_values().to(q.device)[q.long()] * two_e.repeat_interleave(32, dim=1)
    out = v.to(dt)
    assert torch.equal(out.double(), v)
    return out


def exact_operands(c, dev):
    """(A int8 [M, K], ea, codes uint8 [N, K], scale bytes uint8 [N, K / 32], bias fp32 [N], residual fp32 [M, Nout] or None)"""
    g = torch.Generator().manual_seed(c.M * 1000003 + c.N * 1009 + c.K + 7 * c.epi + 4)
    amax = 7 if c.K <= 8192 else 3
    ea2 = 1.0 if c.norm else sum(i * i for i in range(1, amax + 1)) / amax
    t = round(math.log2(math.sqrt(c.K * ea2) * W_RMS))
    base = -min(t, 13)
    ea = 0 if c.norm else t + base
    nout = c.N // 2 if c.epi == R.SILU else c.N
    A = torch.randint(1, amax + 1, (c.M, c.K), generator=g, dtype=torch.int8)
    A = torch.where(torch.randint(0, 2, (c.M, c.K), generator=g, dtype=torch.int8) == 1, A, -A)
    q = torch.randint(0, 16, (c.N, c.K), generator=g, dtype=torch.uint8)
    n, kb = torch.arange(c.N)[:, None], torch.arange(c.K // 32)[None, :]
    s = (127 + base + (n + 7 * kb) % SPREAD).to(torch.uint8)
    bias = torch.randint(-64, 65, (c.N,), generator=g).float() / 32.0
    res = torch.randint(-64, 65, (c.M, nout), generator=g).float() / 32.0 if c.mode == R.F32R else None
    return A.to(dev), ea, q.to(dev), s.to(dev), bias.to(dev), None if res is None else res.to(dev)


def mx4_operand(q, s, N, dt):
    """row-major codes / scale bytes [N, ..] on the GPU -> (dW: panel-tiled dq with NaN pad rows, q4 / s4: the poisoned panels,
    dq [N, K])"""
    dev, Npad, Kk = q.device, R.cdiv(N, 16) * 16, q.shape[1]
    qp = torch.full((Npad, Kk), 7, dtype=torch.uint8, device=dev)
    qp[:N] = q
    sp = torch.full((Npad, Kk // 32), 255, dtype=torch.uint8, device=dev)
    sp[:N] = s
    qbuf = torch.full((Npad * Kk // 2 + 4096,), 0x77, dtype=torch.uint8, device=dev)
    qbuf[:Npad * Kk // 2] = W4.tile(qp).reshape(-1)
    sbuf = torch.full((Npad * Kk // 32 + 64,), 255, dtype=torch.uint8, device=dev)
    sbuf[:Npad * Kk // 32] = W4.tile_scales(sp).reshape(-1)
    dq = _dq(q, s, dt)
    dqp = torch.full((Npad, Kk), float("nan"), dtype=dt, device=dev)
    dqp[:N] = dq
    return tile_weight(dqp), qbuf, sbuf, dq


def launch(ctx, form, A, dW, q4, s4, bias, res_out, out, c, eps=1e-5):
    ks, ran = C.c_int32(-1), C.c_int32(-1)
    _cabi.check(_cabi.lib().opus_debug_gemm_w4(
        ctx, form, A.data_ptr(), dW.data_ptr(), q4.data_ptr(), s4.data_ptr(), None if bias is None else bias.data_ptr(),
        None if res_out is None else res_out.data_ptr(), out.data_ptr(), c.M, c.N, c.K, 0 if form == 2 else c.epi,
        1 if c.mode != R.F16 else 0, eps, C.byref(ks), C.byref(ran), None))
    return ks.value, ran.value


def run_exact_case(ctx, dev, c, repeats=1):
    """The exact operands through opus_debug_gemm_w4.  With the norm fused the activations are the integers as fp32 (the norm
    itself is not exact: held to fp64 within NORM_RULE)."""
    dt = _cabi.operand_dtype()
    nout = c.N // 2 if c.epi == R.SILU else c.N
    out_dt = torch.float32 if c.mode != R.F16 else dt
    Ai, ea, q, s, bias, res = exact_operands(c, dev)
    dW, q4, s4, dq = mx4_operand(q, s, c.N, dt)
    # every code under every one of the SPREAD scale bytes; the fp32 sums are exact
    pairs = torch.bincount((q.long() * 256 + s.long().repeat_interleave(32, dim=1)).reshape(-1), minlength=16 * 256).view(16, 256)
    units = dq.double().abs() * 2.0 ** (128 - int(s.min()))                # |w| in units of half the smallest block scale
    obs = {"id": R.case_id(c), "scales_per_code": int((pairs > 0).sum(1).min()),
           "scale_spread_in_panel": int(s[:16, 0].max()) - int(s[:16, 0].min()), "scale_spread_along_k": int(s[0].max()) - int(s[0].min()),
           "exact_sums": bool((Ai.double().abs() @ units.T).max() + 2 * 2.0 * 2.0 ** (128 - int(s.min()) + ea) < 2.0 ** 24)}
    if c.norm:
        A = K._poisoned(Ai.float(), R.a_rows(c.M))
        bias, res = None, None
        pre, ref = None, R.norm_reference(Ai.float(), dq, c.epi)
    else:
        A16 = (Ai.float() * 2.0 ** -ea).to(dt)
        A = K._poisoned(A16, R.a_rows(c.M))
        if c.slab:
            bias = None
        pre = A16.double() @ dq.double().T + (0.0 if bias is None else bias.double())
        ref = R.activate(pre, R.PLAIN if c.slab else c.epi)
        if res is not None:
            ref = ref + res.double()
    if c.a_tiled:
        A = tile_weight(A)
    A0, W0, q0, s0 = A.clone(), dW.clone(), q4.clone(), s4.clone()
    outs, plans, rans = [], [], []
    lib = _cabi.lib()
    if c.a_tiled:
        _cabi.check(lib.opus_debug_knob(ctx, b"debug_a_tiled", 1))
    try:
        for _ in range(repeats):
            if c.slab:
                out = torch.full((8 * c.M * c.N + R.GUARD_ROWS * c.N,), R.SENTINEL, dtype=torch.float32, device=dev)
                ks, ran = launch(ctx, 2, A, dW, q4, s4, None, None, out, c)
                obs["ks"] = ks
            else:
                out = torch.full((c.M + R.GUARD_ROWS, nout), R.SENTINEL, dtype=out_dt, device=dev)
                if res is not None:
                    out[:c.M] = res
                ks, ran = launch(ctx, 1 if c.norm else 0, A, dW, q4, s4, bias, out if res is not None else None, out, c)
            plans.append(K.report(ctx))
            rans.append(ran)
            outs.append(out)
        torch.cuda.synchronize()
    finally:
        if c.a_tiled:
            _cabi.check(lib.opus_debug_knob(ctx, b"debug_a_tiled", 0))
    obs["plans"] = [list(p) for p in plans]
    obs["ran_w4"] = rans
    obs["repeats_equal"] = all(torch.equal(K._bits(outs[0]), K._bits(o)) for o in outs[1:])
    obs["bystanders_untouched"] = bool(torch.equal(K._bits(A), K._bits(A0)) and torch.equal(K._bits(dW), K._bits(W0)) and
                                       torch.equal(q4, q0) and torch.equal(s4, s0))
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
    """K.failures (route == the case's plan, poison, exactness / the kernel rules) + the MXFP4 assertions."""
    bad = K.failures(c, obs, bf16)
    if not obs["exact_sums"]:
        bad.append("the operands' partial sums can pass 2^24 units: the case is not exact")
    if obs["scales_per_code"] < 8 or obs["scale_spread_in_panel"] < 6 or obs["scale_spread_along_k"] < 6:
        bad.append(f"scales: {obs['scales_per_code']} per code, spread {obs['scale_spread_in_panel']} in a panel, {obs['scale_spread_along_k']} along K")
    want = 1 if c.plan.klass in W4_CLASSES else 0
    if any(r != want for r in obs["ran_w4"]):
        bad.append(f"ran_w4 {obs['ran_w4']}, expected {want}")
    return bad


# ------------------------------------------------------------------------------------------------ Gaussian operands
def run_gaussian_case(ctx, dev, c):
    """gaussian_inputs with the rows of W spread over 15 binades (w8_checks.row_exponent_spread) and the 32-k blocks of a row over
    another 4, through the quantiser; reference: fp64 on (the operand-type A, dq)."""
    dt = _cabi.operand_dtype()
    nout = c.N // 2 if c.epi == R.SILU else c.N
    X, Wg = R.gaussian_inputs(c)
    two = torch.tensor(2.0, dtype=torch.float64)
    Wg = Wg.double() * torch.pow(two, Q.row_exponent_spread(c.N))[:, None]
    Wg = (Wg * torch.pow(two, (torch.arange(c.K) // 32 % 4 - 2).double())[None, :]).to(dt).to(dev)
    Npad = R.cdiv(c.N, 16) * 16
    Wp = torch.zeros((Npad, c.K), dtype=dt, device=dev)
    Wp[:c.N] = Wg
    q4, s4, _ = quantize_mxfp4(Wp)
    q, s = untile_mxfp4(q4, s4)
    dW, q4, s4, dq = mx4_operand(q[:c.N], s[:c.N], c.N, dt)
    sc = s[:c.N].int()
    obs = {"id": R.case_id(c), "scale_spread_in_panel": int(sc[:16, 0].max() - sc[:16, 0].min()),
           "scale_spread_along_k": int(sc[0].max() - sc[0].min()),
           "dq_rel_rms": float(((dq.double() - Wg.double()).norm() / Wg.double().norm()))}
    if c.epi == R.SILU:
        obs["scale_spread_in_pair"] = int((sc[:16, 0] - sc[16:32, 0]).abs().min())
    out_dt = torch.float32 if c.mode != R.F16 else dt
    out = torch.full((c.M + R.GUARD_ROWS, nout), R.SENTINEL, dtype=out_dt, device=dev)
    if c.norm:
        A = K._poisoned(X.to(dev), R.a_rows(c.M))
        ref = R.norm_reference(X.to(dev), dq, c.epi)
        _, ran = launch(ctx, 1, A, dW, q4, s4, None, None, out, c)
    else:
        A16 = X.to(dt).to(dev)
        A = K._poisoned(A16, R.a_rows(c.M))
        ref = R.activate(A16.double() @ dq.double().T, c.epi)
        if c.a_tiled:
            A = tile_weight(A)
            _cabi.check(_cabi.lib().opus_debug_knob(ctx, b"debug_a_tiled", 1))
        try:
            _, ran = launch(ctx, 0, A, dW, q4, s4, None, None, out, c)
        finally:
            if c.a_tiled:
                _cabi.check(_cabi.lib().opus_debug_knob(ctx, b"debug_a_tiled", 0))
    torch.cuda.synchronize()
    obs["plans"] = [list(K.report(ctx))]
    obs["ran_w4"] = [ran]
    obs["guard_untouched"] = bool((out[c.M:] == R.SENTINEL).all())
    got = out[:c.M]
    obs["finite"] = bool(torch.isfinite(got).all())
    obs["err"] = float((got.double() - ref).abs().max())
    obs["ref_max"] = float(ref.abs().max())
    return obs
