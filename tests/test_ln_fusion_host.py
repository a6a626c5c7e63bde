"""CPU checks of tests/ln_fusion_ref.py - the reference the GPU tests of the fused norms (tests/test_gpu_ln_fusion.py) stand on:
the fused form is the norm followed by the GEMM, the weight fold is oracle/esm2.py's LayerNorm followed by Linear, the fp32
emulation walks the sums in the kernels' order, and the error model reproduces the table its bounds are taken from.

Every assertion here was seen to fail against a perturbed reference while it was written: the column sums of column n + 1,
c2 without W beta, gamma left out of the fold, a finalize emulation that walks the slabs in index order where the kernel
interleaves 16 streams (the partials of that test differ in magnitude, so the order shows), a butterfly that pairs lane i with
lane i + 8 first, round16 that truncates, and the model evaluated with the stand-alone rounding point in both columns."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ln_fusion_ref as R
from opus_pllm_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(M=24, K=320, N=192, seed=0, mu=3.0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((M, K)) * 1.7 + mu
    W = rng.standard_normal((N, K)) / np.sqrt(K)
    gamma, beta, b = 1.0 + 0.3 * rng.standard_normal(K), 0.2 * rng.standard_normal(K), 0.1 * rng.standard_normal(N)
    return X, W, gamma, beta, b


@pytest.mark.parametrize("epi", [0, 1])
def test_fused_form_is_norm_then_gemm_in_fp64(epi):
    """rstd (x W'^T - mu s) + c2 == ((x - mu) rstd) W'^T + c2 when nothing is rounded."""
    X, W, gamma, beta, b = _case()
    Wf, c2 = R.fold(W, gamma, beta, b)
    mu, rstd = R.stats_f64(X, 1e-5)
    exact = R.consumer_exact_f64(X, mu, rstd, Wf, c2, epi)
    fused = R.consumer_fused_f64(X, mu, rstd, Wf, R.colsum(Wf), c2, epi)
    assert np.abs(fused - exact).max() <= 1e-12 * np.abs(exact).max()
    # the check has teeth: the neighbour's column sum is a different function
    wrong = R.consumer_fused_f64(X, mu, rstd, Wf, np.roll(R.colsum(Wf), -1), c2, epi)
    assert np.abs(wrong - exact).max() > 1e-3 * np.abs(exact).max()


def test_rms_form_and_gate_up_in_fp64():
    X, W, gamma, _, _ = _case(N=256, mu=0.5)
    Wf, c2 = R.fold(W, gamma, None, None)
    assert c2 is None
    mu, rstd = R.stats_f64(X, 1e-5, rms=True)
    assert not mu.any() and np.allclose(rstd, 1.0 / np.sqrt((X * X).mean(1) + 1e-5), rtol=1e-14)
    for epi in (0, 2):
        exact = R.consumer_exact_f64(X, mu, rstd, Wf, None, epi)
        fused = R.consumer_fused_f64(X, mu, rstd, Wf, None, None, epi)
        assert exact.shape == (X.shape[0], 256 if epi == 0 else 128)
        assert np.abs(fused - exact).max() <= 1e-12 * np.abs(exact).max()
    y = torch.from_numpy((X * rstd[:, None]) @ Wf.T).view(X.shape[0], 8, 2, 16)
    want = (torch.nn.functional.silu(y[:, :, 0]) * y[:, :, 1]).reshape(X.shape[0], 128).numpy()
    assert np.abs(R.consumer_exact_f64(X, mu, rstd, Wf, None, 2) - want).max() < 1e-12


def test_fold_is_the_oracles_layernorm_then_linear():
    """oracle/esm2.py: h = F.layer_norm(x, (D,), ln.weight, ln.bias, eps); gelu_erf(F.linear(h, fc1.weight, fc1.bias))."""
    from oracle.esm2 import gelu_erf
    X, W, gamma, beta, b = _case(seed=4)
    t = lambda a: torch.from_numpy(a)
    h = torch.nn.functional.layer_norm(t(X), (X.shape[1],), t(gamma), t(beta), 1e-5)
    lin = torch.nn.functional.linear(h, t(W), t(b))
    Wf, c2 = R.fold(W, gamma, beta, b)
    mu, rstd = R.stats_f64(X, 1e-5)
    for epi, want in ((0, lin), (1, gelu_erf(lin))):
        got = R.consumer_fused_f64(X, mu, rstd, Wf, R.colsum(Wf), c2, epi)
        assert np.abs(got - want.numpy()).max() <= 1e-12 * float(want.abs().max())
    # torch tensors go through the same functions (the GPU tests use them on the device)
    got_t = R.consumer_fused_f64(t(X), t(mu), t(rstd), t(Wf), t(R.colsum(Wf)), t(c2), 1)
    assert float((got_t - gelu_erf(lin)).abs().max()) <= 1e-12 * float(lin.abs().max())


def test_round16_is_round_to_nearest_even_in_both_types():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(4096) * 50, [6.0e4, 0.0, -0.0, 1.00048828125, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]]).astype(np.float32)
    for bf, dt in ((False, torch.float16), (True, torch.bfloat16)):
        want = torch.from_numpy(x).to(dt).double().numpy()
        assert np.array_equal(R.round16(x, bf), want)
        assert torch.equal(R.round16(torch.from_numpy(x), bf), torch.from_numpy(want))


def _finalize_transcribed(part, nslab, inv_d, eps, rms):
    """ln_finalize_kernel for one row, statement by statement, in np.float32 scalars: 16 lanes, then the xor butterfly."""
    f = np.float32
    s1, s2 = [f(0)] * 16, [f(0)] * 16
    for q in range(16):
        for j0 in range(0, nslab, 64):
            t = []
            for u in range(4):
                j = j0 + 16 * u + q
                t.append(part[j] if j < nslab else (f(0), f(0)))
            s1[q] = f(s1[q] + f(f(t[0][0] + t[1][0]) + f(t[2][0] + t[3][0])))
            s2[q] = f(s2[q] + f(f(t[0][1] + t[1][1]) + f(t[2][1] + t[3][1])))
    for o in (1, 2, 4, 8):
        s1 = [f(s1[q] + s1[q ^ o]) for q in range(16)]
        s2 = [f(s2[q] + s2[q ^ o]) for q in range(16)]
    if rms:
        return f(0), f(1) / np.sqrt(f(f(s2[0] * inv_d) + eps))
    mu = f(s1[0] * inv_d)
    var = max(f(f(s2[0] * inv_d) - f(mu * mu)), f(0))
    return mu, f(1) / np.sqrt(f(var + eps))


@pytest.mark.parametrize("nslab", [20, 40, 64, 80])
def test_finalize_emulation_walks_the_slabs_as_the_kernel_does(nslab):
    rng = np.random.default_rng(nslab)
    # partials of very different magnitude: any other summation order gives other bits
    s1 = (rng.standard_normal((6, nslab)) * 10.0 ** rng.integers(-3, 4, (6, nslab))).astype(np.float32)
    s2 = (rng.random((6, nslab)) * 10.0 ** rng.integers(-3, 4, (6, nslab))).astype(np.float32)
    D, eps = nslab * 64, np.float32(1e-5)
    for rms in (False, True):
        mu, rstd = R.finalize_f32(s1, s2, D, 1e-5, rms)
        for r in range(6):
            m, rs = _finalize_transcribed([(s1[r, j], s2[r, j]) for j in range(nslab)], nslab, np.float32(1.0) / np.float32(D), eps, rms)
            assert mu[r] == m
            assert abs(float(rstd[r]) - float(rs)) <= 2.0 ** -23 * float(rs)       # (x ** -0.5 against 1 / sqrt(x): one ulp)
    # ... and on torch tensors
    mu_t, rstd_t = R.finalize_f32(torch.from_numpy(s1), torch.from_numpy(s2), D, 1e-5)
    mu_n, rstd_n = R.finalize_f32(s1, s2, D, 1e-5)
    assert np.array_equal(mu_t.numpy(), mu_n) and np.allclose(rstd_t.numpy(), rstd_n, rtol=3e-7)


def test_partial_emulation_order_and_accuracy():
    rng = np.random.default_rng(7)
    X = (rng.standard_normal((5, 256)) * 10.0 ** rng.integers(-2, 3, (5, 256))).astype(np.float32)
    s1, s2 = R.partials_f32(X)
    f = np.float32
    for r in range(5):
        for sl in range(4):
            lane1, lane2 = [], []
            for l in range(16):
                v = X[r, sl * 64 + 4 * l: sl * 64 + 4 * l + 4]
                lane1.append(f(f(v[0] + v[1]) + f(v[2] + v[3])))
                lane2.append(f(f(f(v[0] * v[0]) + f(v[1] * v[1])) + f(f(v[2] * v[2]) + f(v[3] * v[3]))))
            for o in (1, 2, 4, 8):
                lane1 = [f(lane1[q] + lane1[q ^ o]) for q in range(16)]
                lane2 = [f(lane2[q] + lane2[q ^ o]) for q in range(16)]
            assert len(set(lane1)) == 1 and len(set(lane2)) == 1       # every lane of the butterfly ends with the same bits
            assert s1[r, sl] == lane1[0] and s2[r, sl] == lane2[0]
    r1, r2 = R.partials_f64(X.astype(np.float64))
    a1, a2 = R.partial_scales_f64(X.astype(np.float64))
    assert np.array_equal(a1, np.abs(X.astype(np.float64)).reshape(5, 4, 64).sum(2))
    w1, w2 = R.emulated_partial_error(X)
    # a 64-term fp32 sum as a depth-6 tree (+ the squares' own rounding): at most 7 half-ulps of the sum of magnitudes
    assert 0 < w1 <= 7 * 2.0 ** -24 and 0 < w2 <= 8 * 2.0 ** -24
    t1, t2 = R.partials_f32(torch.from_numpy(X))
    assert np.array_equal(t1.numpy(), s1) and np.array_equal(t2.numpy(), s2)


@pytest.mark.parametrize("bf16", [False, True])
def test_error_model_reproduces_the_table(bf16):
    """K = 1280, unit-variance rows, folded 16-bit weights: the fused form's error grows with |mu| / sigma (it rounds x where
    the stand-alone form rounds (x - mu) rstd), the stand-alone form's does not.  Maxima over 256 x 1280 outputs of another
    sample than the table's: within a factor 1.5."""
    Wf, c2 = R.model_weights(1280, 1280, 1, bf16)
    got = {}
    for m, row in R.MODEL_TABLE.items():
        e = R.model_errors(R.model_rows(256, 1280, m, 100 + m), Wf, c2, 1e-5, bf16)
        got[m] = e
        want_f, want_s = row[2 * bf16], row[2 * bf16 + 1]
        assert want_f / 1.5 <= e["fused"] <= want_f * 1.5, (m, e, want_f)
        assert want_s / 1.5 <= e["standalone"] <= want_s * 1.5, (m, e, want_s)
        if m in R.MODEL_RSTD:
            assert R.MODEL_RSTD[m] / 2 <= e["rstd"] <= R.MODEL_RSTD[m] * 2, (m, e)
    assert got[0]["fused"] < 1.2 * got[0]["standalone"]                 # no mean: the two forms round the same numbers
    assert got[64]["fused"] > 30 * got[64]["standalone"]                # |mu| = 64 sigma: 6 bits of the hand-off are spent on mu


def test_emulated_stat_error_scales_with_the_mean():
    """E[x^2] - mu^2 in fp32: the variance's relative error grows as 1 + mu^2 / var, and so does the bound the GPU test takes."""
    worst = {}
    for m in (0, 8, 64):
        em, er = R.emulated_stat_error(R.model_rows(64, 1280, m, 5 + m), 1e-5)
        worst[m] = (float(em.max()), float(er.max()))
        assert worst[m][0] < 4e-7                                       # mu itself is a plain sum: a few ulps at any mean
    assert worst[0][1] < 1e-6 < 10 * worst[8][1] and worst[8][1] < 1e-4 < worst[64][1] < 5e-3, worst
    # var = 0: eps decides, and the cancellation noise of E[x^2] - mu^2 is measured against it
    const = np.full((2, 1280), 0.75, dtype=np.float32)
    em, er = R.emulated_stat_error(const, 1e-5)
    assert float(em.max()) < 2e-7 and float(er.max()) < 5e-3
    zero = np.zeros((2, 1280), dtype=np.float32)
    em, er = R.emulated_stat_error(zero, 1e-5)
    assert float(em.max()) == 0.0 and float(er.max()) <= 3 * 2.0 ** -23


def test_new_symbol_is_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "opus_pllm.h")).read(), flags=re.S)
    lib = _cabi.lib()
    name = "opus_debug_gemm_ln"
    m = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr)
    assert m and m.group(1).count(",") + 1 == 24
    assert len(_cabi.SIGNATURES[name][1]) == 24
    fn = getattr(lib, name)
    assert fn.restype == ctypes.c_int and fn.argtypes == _cabi.SIGNATURES[name][1]
    assert lib.opus_abi_version() == 10
    bf = ctypes.CDLL(os.path.join(os.path.dirname(_cabi.LIB_PATH), "libopus_pllm_bf16.so"))
    assert bf.opus_debug_gemm_ln is not None
    # arguments are checked before anything touches the device
    assert lib.opus_debug_gemm_ln(*([None] * 12), 256, 1280, 1280, 1280, 0, 0, 1e-5, 0, None, None, None, None) == -1
