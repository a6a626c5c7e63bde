"""One case of tests/gemm_cells_ref.py on the GPU (shared by tests/test_gpu_gemm_cells.py and the bf16 child
tests/bf16_gemm_cells_check.py).  run_case() launches the case through opus_debug_gemm / opus_debug_gemm_norm /
opus_debug_gemm_slabs on a poisoned layout and returns what was observed; failures() holds the observations to the case's plan
and to the reference.  Not product code.

Poisoned layout: A is the first M rows of a buffer whose following rows (up to the largest row tile a kernel at this M works on)
are NaN; the padded rows N .. Npad - 1 of W are NaN; the output has GUARD_ROWS sentinel rows behind row M - 1; the residual of the
fp32 + residual mode is the output itself (as the path issues it), so there is no separate residual buffer to watch.
"""
from __future__ import annotations

import ctypes as C

import torch

import gemm_cells_ref as R
from opus_pllm_amd import _cabi
from opus_pllm_amd.weights import tile_weight

REPEATS = 4                        # launches of a cell whose k-parts are combined inside the launch


def make_ctx(cfg, dev):
    ctx = C.c_void_p()
    cc = _cabi.CConfig.from_config(cfg)
    _cabi.check(_cabi.lib().opus_ctx_create(C.byref(cc), dev.index or 0, C.byref(ctx)))
    return ctx


def class_names():
    buf = C.create_string_buffer(512)
    _cabi.check(_cabi.lib().opus_timing_names(buf, 512))
    return buf.value.decode().split(";")[0].split(",")


def report(ctx):
    """the launchers' report of the context's last GEMM as a gemm_cells_ref.Plan (kernel class by name)"""
    w = (C.c_int32 * 8)()
    _cabi.check(_cabi.lib().opus_debug_gemm_plan(ctx, w))
    names = class_names()
    return R.Plan(names[w[0]] if 0 <= w[0] < len(names) else str(w[0]), *list(w)[1:])


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _poisoned(t, rows):
    buf = torch.full((rows, t.shape[1]), float("nan"), dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf


def run_case(ctx, dev, c, repeats=None):
    lib, dt = _cabi.lib(), _cabi.operand_dtype()
    nout = c.N // 2 if c.epi == R.SILU else c.N
    f32 = c.mode != R.F16
    out_dt = torch.float32 if f32 else dt
    obs = {"id": R.case_id(c)}
    if c.norm:
        X, W = R.gaussian_inputs(c)
        W = W.to(dt).to(dev)
        A = _poisoned(X.to(dev), R.a_rows(c.M))
        bias, res, e = None, None, 0
        ref = R.norm_reference(X.to(dev), W, c.epi)
        pre = None
    else:
        Ai, Wi, bi, ri, e = R.exact_inputs(c)
        Ai, Wi, bi = Ai.to(dev), Wi.to(dev), bi.to(dev)
        ri = None if ri is None else ri.to(dev)
        A = _poisoned(Ai.to(dt), R.a_rows(c.M))
        W = (Wi.float() * 2.0 ** -e).to(dt)
        assert torch.equal(W.double(), Wi.double() * 2.0 ** -e)          # the scaled integers are exact in the operand type
        bias = None if c.slab else bi.float() * 2.0 ** -e
        res = None if ri is None else ri.float() * 2.0 ** -e
        pre, ref = R.exact_reference(Ai, Wi, torch.zeros_like(bi) if c.slab else bi, ri, e, R.PLAIN if c.slab else c.epi)
        del Ai, Wi
    Wp = _poisoned(W, R.cdiv(c.N, 16) * 16)
    dW = tile_weight(Wp)
    del Wp, W
    if c.a_tiled:
        A = tile_weight(A)
    A0, W0, b0 = A.clone(), dW.clone(), None if bias is None else bias.clone()
    reps = repeats if repeats is not None else (REPEATS if c.plan.combine in (R.IN_LAUNCH, R.PP_PAIR) else 1)
    outs, plans = [], []
    if c.a_tiled:
        _cabi.check(lib.opus_debug_knob(ctx, b"debug_a_tiled", 1))
    try:
        for _ in range(reps):
            if c.slab:
                out = torch.full((8 * c.M * c.N + R.GUARD_ROWS * c.N,), R.SENTINEL, dtype=torch.float32, device=dev)
                ks = C.c_int32(-1)
                _cabi.check(lib.opus_debug_gemm_slabs(ctx, A.data_ptr(), dW.data_ptr(), out.data_ptr(), c.M, c.N, c.K, C.byref(ks), None))
                obs["ks"] = ks.value
            else:
                out = torch.full((c.M + R.GUARD_ROWS, nout), R.SENTINEL, dtype=out_dt, device=dev)
                if res is not None:
                    out[:c.M] = res                                   # in-place residual accumulate, as the path uses it
                if c.norm:
                    _cabi.check(lib.opus_debug_gemm_norm(ctx, A.data_ptr(), dW.data_ptr(), out.data_ptr(), c.M, c.N, c.K, c.epi,
                                                         1 if f32 else 0, 1e-5, None))
                else:
                    _cabi.check(lib.opus_debug_gemm(ctx, A.data_ptr(), dW.data_ptr(), bias.data_ptr(),
                                                    out.data_ptr() if res is not None else None, out.data_ptr(), c.M, c.N, c.K, c.epi,
                                                    1 if f32 else 0, None))
            plans.append(report(ctx))
            outs.append(out)
        torch.cuda.synchronize()
    finally:
        if c.a_tiled:
            _cabi.check(lib.opus_debug_knob(ctx, b"debug_a_tiled", 0))
    obs["plans"] = [list(p) for p in plans]
    obs["repeats_equal"] = all(torch.equal(_bits(outs[0]), _bits(o)) for o in outs[1:])
    obs["bystanders_untouched"] = bool(torch.equal(_bits(A), _bits(A0)) and torch.equal(_bits(dW), _bits(W0)) and
                                       (bias is None or torch.equal(_bits(bias), _bits(b0))))
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


def bound(c, obs, bf16=False):
    slope, floor = R.NORM_RULE if c.norm else R.KERNEL_RULE
    return (R.BF16_FACTOR if bf16 else 1) * slope * obs["ref_max"] + floor


def failures(c, obs, bf16=False):
    bad = []
    want = list(c.plan)
    if any(p != want for p in obs["plans"]):
        bad.append(f"route: launched {obs['plans'][0]}, filed under {want}")
    if c.slab and obs["ks"] != c.plan.ks:
        bad.append(f"slabs: {obs['ks']} reported, {c.plan.ks} expected")
    for k in ("finite", "guard_untouched", "bystanders_untouched", "repeats_equal"):
        if not obs[k]:
            bad.append(k)
    if "exact" in obs:
        if not obs["exact"]:
            bad.append(f"not bit-exact: {obs.get('n_diff')} elements differ, max |err| {obs.get('err')}")
    elif not obs["err"] <= bound(c, obs, bf16):
        bad.append(f"max |err| {obs['err']} > {bound(c, obs, bf16)}")
    return bad
