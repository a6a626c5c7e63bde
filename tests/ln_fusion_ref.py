"""Reference arithmetic of the norms fused around gemm_pp_kernel (GemmParams::ln_part / ln_stat / ln_colsum), for
tests/test_ln_fusion_host.py (CPU) and tests/test_gpu_ln_fusion.py / tests/bf16_check.py (GPU).  Not product code.

The chain under test (opus_debug_gemm_ln issues it as the encoder and the decoder prefill do):
    X  <- X + A W1^T (+ b1)                     fp32; the GEMM also leaves xh = round16(X) and per-64-column (sum x, sum x^2)
    (mu, rstd) = finalize(partials)             fp32, E[x^2] - mu^2
    C  = epi(rstd (xh W'^T - mu s) + c2)        W' = W diag(gamma), c2 = W beta + b, s[n] = sum_k W'[n][k]
against  C* = epi(LN(X) W^T + b)  with LN(x) = (x - mu) rstd gamma + beta.

Everything here is written with +, -, *, slicing and reshape only, so that the same functions take NumPy arrays (host tests)
and torch tensors on any device (GPU tests: fp64 on the device, as the 4 GiB GEMM test does).  "f64" functions expect float64
inputs; "f32" functions emulate the kernels' fp32 arithmetic in the kernels' own summation order.
"""
from __future__ import annotations

import numpy as np

SLAB = 64            # columns per partial (GemmParams::ln_part)
ULP32 = 2.0 ** -23   # rsqrtf is a 1-ulp function; a correctly rounded emulation cannot reproduce which way it errs


# ------------------------------------------------------------------------------------------------ small array-module shims
def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _f32(x):
    if _is_torch(x):
        import torch
        return x.to(torch.float32)
    return np.asarray(x, dtype=np.float32)


def _f64(x):
    if _is_torch(x):
        import torch
        return x.to(torch.float64)
    return np.asarray(x, dtype=np.float64)


def _zeros_like_cols(x, cols):
    if _is_torch(x):
        import torch
        return torch.zeros(x.shape[0], cols, dtype=x.dtype, device=x.device)
    return np.zeros((x.shape[0], cols), dtype=x.dtype)


def _cat1(a, b):
    if _is_torch(a):
        import torch
        return torch.cat([a, b], 1)
    return np.concatenate([a, b], 1)


def _maximum0(x):
    if _is_torch(x):
        return x.clamp_min(0)
    return np.maximum(x, 0)


def _amax(x):
    return float(x.abs().max()) if _is_torch(x) else float(np.abs(x).max())


def round16(x, bf16: bool = False):
    """x (fp32 / fp64) rounded to the build's 16-bit operand type (round to nearest even), returned as float64."""
    if _is_torch(x):
        import torch
        return x.to(torch.float32).to(torch.bfloat16 if bf16 else torch.float16).to(torch.float64)
    x32 = np.asarray(x, dtype=np.float32)
    if not bf16:
        return x32.astype(np.float16).astype(np.float64)
    u = x32.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the weight fold
def fold(W, gamma, beta, b):
    """(W' = W diag(gamma), c2 = W beta + b) in fp64 from fp64 W [N,K], gamma / beta [K] (None: RMSNorm has no beta), b [N] or None."""
    Wf = W * gamma[None, :]
    c2 = None
    if beta is not None:
        c2 = W @ beta
    if b is not None:
        c2 = b if c2 is None else c2 + b
    return Wf, c2


def colsum(Wf16):
    """s[n] = sum_k W'[n][k] of the folded weight AS STORED (its 16-bit values, summed in fp64)."""
    return Wf16.sum(1)


# ------------------------------------------------------------------------------------------------ the three stages in fp64
def producer_f64(X0, A, W1, b1=None):
    """X = X0 + A W1^T (+ b1)."""
    X = X0 + A @ W1.T
    return X if b1 is None else X + b1[None, :]


def stats_f64(X, eps, rms=False):
    """(mu, rstd) of every row: LayerNorm's (biased variance, as torch) or RMSNorm's (0, rsqrt(mean x^2 + eps))."""
    if rms:
        return X[:, 0] * 0.0, ((X * X).mean(1) + eps) ** -0.5
    mu = X.mean(1)
    d = X - mu[:, None]
    return mu, ((d * d).mean(1) + eps) ** -0.5


def partials_f64(X):
    """(sum x, sum x^2) of every 64-column slab: two [M, N/64] arrays."""
    g = X.reshape(X.shape[0], X.shape[1] // SLAB, SLAB)
    return g.sum(2), (g * g).sum(2)


def partial_scales_f64(X):
    """What a partial's rounding error is measured against: (sum |x|, sum x^2) of the slab."""
    g = X.reshape(X.shape[0], X.shape[1] // SLAB, SLAB)
    return (g * ((g > 0) * 2.0 - 1.0)).sum(2), (g * g).sum(2)


def apply_epi(y, epi):
    """EPI_NONE / EPI_GELU (erf form) / EPI_SILU_GU16 (rows of W in 32-row groups [16 gate | 16 up]) on fp64 y [M,N]."""
    if epi == 0:
        return y
    if _is_torch(y):
        import torch
        if epi == 1:
            return torch.nn.functional.gelu(y)
        r = y.reshape(y.shape[0], y.shape[1] // 32, 2, 16)
        return (torch.nn.functional.silu(r[:, :, 0]) * r[:, :, 1]).reshape(y.shape[0], y.shape[1] // 2)
    from math import erf
    if epi == 1:
        return 0.5 * y * (1.0 + np.vectorize(erf)(y / np.sqrt(2.0)))
    r = y.reshape(y.shape[0], y.shape[1] // 32, 2, 16)
    return (r[:, :, 0] / (1.0 + np.exp(-r[:, :, 0])) * r[:, :, 1]).reshape(y.shape[0], y.shape[1] // 2)


def consumer_exact_f64(X, mu, rstd, Wf, c2, epi=0):
    """Norm first, then the GEMM: epi(((x - mu) rstd) W'^T + c2) - the function the fused form stands for."""
    y = ((X - mu[:, None]) * rstd[:, None]) @ Wf.T
    if c2 is not None:
        y = y + c2[None, :]
    return apply_epi(y, epi)


def consumer_fused_f64(xh, mu, rstd, Wf, s, c2, epi=0):
    """The kernel's own algebra in fp64: epi(rstd (xh W'^T - mu s) + c2); s = None: RMSNorm (mu = 0)."""
    acc = xh @ Wf.T
    if s is not None:
        acc = acc - mu[:, None] * s[None, :]
    y = rstd[:, None] * acc
    if c2 is not None:
        y = y + c2[None, :]
    return apply_epi(y, epi)


def rope_f64(y16, pos, D, cos, sin, qscale):
    """ESM rotary on the fp64 image of an fp16 QKV projection y16 [M, 3 D] (heads of 64, pairs (d, d + 32)): q third scaled by
    qscale first, q and k rotated by the angle of pos[m]; cos / sin [T, 32] fp64 (the fp32 table's values)."""
    out = y16 * 1.0
    M = y16.shape[0]
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    for part, sc in ((0, qscale), (1, 1.0)):
        x = (y16[:, part * D:(part + 1) * D] * sc).reshape(M, D // 64, 64)
        a, b = x[..., :32], x[..., 32:]
        lo, hi = a * c - b * s, b * c + a * s
        out[:, part * D:(part + 1) * D] = _cat_last(lo, hi).reshape(M, D)
    return out


def _cat_last(lo, hi):
    if _is_torch(lo):
        import torch
        return torch.cat([lo, hi], -1)
    return np.concatenate([lo, hi], -1)


# ------------------------------------------------------------------------------------------------ fp32 emulation, kernel order
def _tree16(v):
    """The 16-lane xor butterfly (offsets 1, 2, 4, 8): a balanced tree over the last axis; every lane ends with the same bits."""
    for _ in range(4):
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _fl32(x64):
    """One rounding of an fp64 intermediate to fp32 (what a fused multiply-add does to its exact result)."""
    return _f32(x64)


def partials_f32(X32, fma: bool = False):
    """The producer epilogue's partials in its order: a lane owns 4 consecutive columns, (x0 + x1) + (x2 + x3) and the same over
    the squares, then the 16 lanes of the slab through the butterfly.  fma: the squares contracted the way the compiler may,
    fl(x0 x0 + fl(x1 x1)) - one rounding less per pair."""
    X32 = _f32(X32)
    M, N = X32.shape
    g = X32.reshape(M, N // SLAB, 16, 4)
    s1 = (g[..., 0] + g[..., 1]) + (g[..., 2] + g[..., 3])
    if fma:
        g64 = _f64(g)
        q = _f64(g * g)
        s2 = _fl32(g64[..., 0] * g64[..., 0] + q[..., 1]) + _fl32(g64[..., 2] * g64[..., 2] + q[..., 3])
    else:
        q = g * g
        s2 = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    return _tree16(s1), _tree16(s2)


def _finalize_sums_f32(p32):
    """ln_finalize_kernel's sum over a row's slabs: 16 lanes, lane q takes slabs q, q + 16, q + 32, q + 48 of every group of 64
    as (t0 + t1) + (t2 + t3) added to its running sum, then the 16-lane butterfly."""
    p32 = _f32(p32)
    M, n = p32.shape
    pad = -n % 64
    if pad:
        p32 = _cat1(p32, _zeros_like_cols(p32, pad))
    g = p32.reshape(M, (n + pad) // 64, 4, 16)
    acc = _zeros_like_cols(p32, 16)
    for j in range(g.shape[1]):
        acc = acc + ((g[:, j, 0] + g[:, j, 1]) + (g[:, j, 2] + g[:, j, 3]))
    return _tree16(acc)


def finalize_f32(s1_32, s2_32, D, eps, rms=False, variant=0):
    """(mu, rstd) in fp32 from fp32 partials, as ln_finalize_kernel: mu = S1 / D, var = max(S2 / D - mu^2, 0), rsqrt(var + eps).
    variant: how the compiler may contract var - 0 none, 1 fma(S2, 1/D, -fl(mu mu)), 2 fma(-mu, mu, fl(S2 / D))."""
    t1, t2 = _finalize_sums_f32(s1_32), _finalize_sums_f32(s2_32)
    inv_d = np.float32(1.0) / np.float32(D)
    eps32 = float(np.float32(eps))
    if rms:
        if variant == 1:
            v = _fl32(_f64(t2) * float(inv_d) + eps32)
        else:
            v = t2 * float(inv_d) + eps32 if _is_torch(t2) else (t2 * inv_d + np.float32(eps32)).astype(np.float32)
        return t1 * 0, _f32(_f32(v) ** -0.5)
    mu = _f32(t1 * float(inv_d)) if _is_torch(t1) else (t1 * inv_d).astype(np.float32)
    e2 = _f32(t2 * float(inv_d)) if _is_torch(t2) else (t2 * inv_d).astype(np.float32)
    if variant == 0:
        var = e2 - mu * mu
    elif variant == 1:
        var = _fl32(_f64(t2) * float(inv_d) - _f64(mu * mu))
    else:
        var = _fl32(_f64(e2) - _f64(mu) * _f64(mu))
    var = _maximum0(_f32(var))
    v = var + eps32 if _is_torch(var) else (var + np.float32(eps32)).astype(np.float32)
    return mu, _f32(_f32(v) ** -0.5)


VARIANTS = (0, 1, 2)


def stat_errors(mu, rstd, mu_ref, rstd_ref, sigma_ref):
    """How (mu, rstd) errors are measured: |mu - mu*| against (|mu*| + sigma*) of the row, rstd relative.  Arrays in, arrays out."""
    den = _f64(mu_ref) * ((_f64(mu_ref) > 0) * 2.0 - 1.0) + _f64(sigma_ref)
    dm = _f64(mu) - _f64(mu_ref)
    dm = dm * ((dm > 0) * 2.0 - 1.0)
    tiny = 1e-300
    em = dm / (den + tiny)
    dr = _f64(rstd) - _f64(rstd_ref)
    dr = dr * ((dr > 0) * 2.0 - 1.0)
    return em, dr / _f64(rstd_ref)


def emulated_stat_error(X32, eps, rms=False):
    """Worst (mu, rstd) error of the fp32 emulation over every contraction variant, per row, against fp64 of the same X32 -
    plus one ulp on rstd for rsqrtf.  Returns (err_mu [M], err_rstd [M])."""
    X64 = _f64(X32)
    mu_r, rstd_r = stats_f64(X64, eps, rms)
    sig = ((X64 - X64.mean(1)[:, None]) ** 2).mean(1) ** 0.5
    worst_m = worst_r = None
    for fma in (False, True):
        s1, s2 = partials_f32(X32, fma)
        for v in VARIANTS:
            mu, rstd = finalize_f32(s1, s2, X32.shape[1], eps, rms, v)
            em, er = stat_errors(mu, rstd, mu_r, rstd_r, sig)
            worst_m = em if worst_m is None else _emax(worst_m, em)
            worst_r = er if worst_r is None else _emax(worst_r, er)
    return worst_m, worst_r + ULP32


def _emax(a, b):
    if _is_torch(a):
        import torch
        return torch.maximum(a, b)
    return np.maximum(a, b)


def emulated_partial_error(X32):
    """Worst error of the emulated partials over both contraction variants, measured as the tests measure the device's:
    |partial - fp64 partial| / (sum |x| resp. sum x^2) of the slab.  Returns (worst of sum x, worst of sum x^2) as floats."""
    X64 = _f64(X32)
    r1, r2 = partials_f64(X64)
    a1, a2 = partial_scales_f64(X64)
    w1 = w2 = 0.0
    for fma in (False, True):
        s1, s2 = partials_f32(X32, fma)
        w1 = max(w1, _amax((_f64(s1) - r1) / (a1 + 1e-300)))
        w2 = max(w2, _amax((_f64(s2) - r2) / (a2 + 1e-300)))
    return w1, w2


# ------------------------------------------------------------------------------------------------ the host error model
def model_rows(n_rows, K, mu_over_sigma, seed):
    """Unit-variance rows with the given mean: x = mu + z, z ~ N(0, 1) (fp32 values, as the residual stream holds them)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_rows, K)) + mu_over_sigma).astype(np.float32)


def model_weights(N, K, seed, bf16=False):
    """A folded weight as the library stores it: W' = W diag(gamma) rounded to 16 bits (fp64 image), c2 = W beta + b (fp64)."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((N, K)) / np.sqrt(K)
    gamma = 1.0 + 0.1 * rng.standard_normal(K)
    beta = 0.1 * rng.standard_normal(K)
    b = 0.1 * rng.standard_normal(N)
    Wf, c2 = fold(W, gamma, beta, b)
    return round16(Wf, bf16), c2


def model_errors(X32, Wf16, c2, eps, bf16=False, rms=False, epi=0):
    """The error model of the fusion on rows X32 (any array module): max |form - exact| / max |exact| of
      fused       rstd32 (round16(x) W'^T - mu32 s) + c2, (mu32, rstd32) from the fp32 emulation, evaluated in fp64;
      standalone  round16((x - mu) rstd) W'^T + c2 (what the stand-alone norm kernel hands to a plain GEMM),
    both before the output's own 16-bit rounding, and the emulation's relative rstd error.  exact = fp64 norm, then GEMM."""
    X64 = _f64(X32)
    mu, rstd = stats_f64(X64, eps, rms)
    exact = consumer_exact_f64(X64, mu, rstd, Wf16, c2, epi)
    s1, s2 = partials_f32(X32)
    mu32, rstd32 = finalize_f32(s1, s2, X32.shape[1], eps, rms)
    fused = consumer_fused_f64(round16(X32, bf16), _f64(mu32), _f64(rstd32), Wf16, None if rms else colsum(Wf16), c2, epi)
    xn = round16((X64 - mu[:, None]) * rstd[:, None], bf16)
    alone = xn @ Wf16.T
    if c2 is not None:
        alone = alone + c2[None, :]
    alone = apply_epi(alone, epi)
    scale = _amax(exact)
    return dict(fused=_amax(fused - exact) / scale, standalone=_amax(alone - exact) / scale,
                fused_abs=_amax(fused - exact), rstd=_amax((_f64(rstd32) - rstd) / rstd), scale=scale)


# The table of the issue this module was written for (fp64 CPU model, K = 1280, unit-variance rows, folded 16-bit weights):
# mu / sigma -> (fp16 fused, fp16 stand-alone, bf16 fused, bf16 stand-alone), max error relative to max |ref|, and the relative
# error of the fp32 rstd.  tests/test_ln_fusion_host.py holds model_errors() to it.
MODEL_TABLE = {0: (2.3e-4, 2.2e-4, 1.6e-3, 1.6e-3), 1: (2.9e-4, 2.0e-4, 2.5e-3, 1.7e-3), 8: (1.8e-3, 2.1e-4, 1.5e-2, 1.6e-3),
               64: (1.2e-2, 1.6e-4, 1.25e-1, 1.7e-3)}
MODEL_RSTD = {0: 1.5e-7, 8: 1.4e-5, 64: 7.8e-4}
