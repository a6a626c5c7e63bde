"""One case of the fused-norm chain on the GPU, measured against fp64 (shared by tests/test_gpu_ln_fusion.py and the bf16 child
tests/bf16_check.py; the arithmetic is tests/ln_fusion_ref.py).  run_case() drives opus_debug_gemm_ln on one shape and returns
every figure the tests assert together with the bound it is held to; check_case() asserts them.  Not product code.

Row statistics.  Rows are dealt to classes by row % 16, so every row tile, every tail tile and the ragged last tile hold all
of them:  0-3 mu / sigma = 0,  4-6 = 1,  7-9 = 8,  10-12 = 64  (x = sigma z + mu, sigma^2 = 1.25),  13 one entry at 6.0e4 (finite in
fp16),  14 all zero,  15 constant 0.75 (var = 0: eps decides).  Rows 14 / 15 have a zero A row, so X is exactly that after the
producer (cases with a producer bias b1 shift them by b1; they are ordinary rows there).  Values beyond the fp16 range are out of
scope for the fp16 build: the un-normalised fp16(x) hand-off cannot represent them.
"""
from __future__ import annotations

import ctypes as C

import torch

import ln_fusion_ref as R
from opus_pllm_amd import _cabi
from opus_pllm_amd.weights import tile_weight

CLASSES = ("r0", "r1", "r8", "r64", "big", "zero", "const")
CLASS_OF_ROW = (0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 5, 6)
RATIO = {0: 0.0, 1: 1.0, 2: 8.0, 3: 64.0}
SENTINEL = -12345.0
PAD_ROWS = 64                      # rows behind M in part / xh / stat / C: pre-filled, must come back untouched
NONE, PAIR, REDUCE = 0, 1, 2
EPS_LN, EPS_RMS = 1e-5, 1e-5
OUT_RULE = (2e-3, 1e-5)            # the project's kernel rule, fp16 output: 2e-3 max |ref| + 1e-5 (tests/test_gpu_parity.py::test_gemm_kernels)
ROPE_RULE = 3e-3                   # test_fused_rotary_epilogue_is_the_standalone_kernel: 3e-3 max |ref| (the rounding to fp16 in front of the rotation moves both neighbours)
BF16_FACTOR = 8                    # tests/test_gpu_bf16.py: bf16 has 8 significand bits against fp16's 11


def make_ctx(cfg, dev):
    ctx = C.c_void_p()
    cc = _cabi.CConfig.from_config(cfg)
    _cabi.check(_cabi.lib().opus_ctx_create(C.byref(cc), dev.index or 0, C.byref(ctx)))
    return ctx


def rope_table(T, theta, dev):
    """(cos, sin) [T, 32] as the library's table holds them: fp32 inv_freq, fp32 angle, evaluated in double, stored as fp32."""
    inv = 1.0 / torch.pow(torch.tensor(theta, dtype=torch.float32), torch.arange(0, 64, 2, dtype=torch.float32) / 64.0)
    ang = (torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]).double()
    return ang.cos().float().double().to(dev), ang.sin().float().double().to(dev)


def _class_masks(M, dev):
    cls = torch.tensor(CLASS_OF_ROW, device=dev)[torch.arange(M, device=dev) % 16]
    return [cls == i for i in range(len(CLASSES))]


def run_case(ctx, dev, M, N1, K1, N2, epi=0, rms=False, rope=None, b1=False, seed=0, repeats=0, standalone=True, rope_theta=10000.0,
             rope_T=514):
    """rope: None / "row" (position = row % rope_T) / "pos" (a row -> position table, the token-packed form)."""
    lib = _cabi.lib()
    bf16 = _cabi.BF16
    dt = _cabi.operand_dtype()
    eps = EPS_RMS if rms else EPS_LN
    g = torch.Generator(device=dev).manual_seed(1000 * seed + M % 997 + N2)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    masks = _class_masks(M, dev)
    # ---- operands
    A = (rnd(M, K1) * 0.5)
    A[masks[5] | masks[6]] = 0.0
    A = A.to(dt)
    W1 = (rnd(N1, K1) / K1 ** 0.5).to(dt)
    bias1 = (rnd(N1) * 0.1) if b1 else None
    X0 = rnd(M, N1)
    for c, ratio in RATIO.items():
        X0[masks[c]] += ratio * 1.25 ** 0.5
    big_rows = masks[4].nonzero().flatten()
    X0[big_rows, (big_rows * 37) % N1] = 6.0e4
    X0[masks[5]] = 0.0
    X0[masks[6]] = 0.75
    W = rnd(N2, N1).double() / N1 ** 0.5
    gamma = 1.0 + 0.1 * rnd(N1).double()
    gu = epi == 2
    beta = None if rms else 0.1 * rnd(N1).double()
    b2 = None if gu else 0.1 * rnd(N2).double()
    Wf, c2 = R.fold(W, gamma, beta, b2)
    Wf16_t = Wf.float().to(dt)                                   # the folded weight as the library stores it
    Wf16 = Wf16_t.double()
    s32 = None if rms else Wf16_t.float().sum(1)                 # weights.py: fp32 row sums of the folded, rounded weight
    c2_32 = None if c2 is None else c2.float()
    del W, Wf
    dW1, dW2 = tile_weight(W1.contiguous()), tile_weight(Wf16_t.contiguous())
    nslab, nout = N1 // 64, N2 // 2 if gu else N2
    pos = None
    if rope == "pos":                                            # packed proteins of 37 .. 1000 tokens back to back
        lens, tot = [], 0
        while tot < M:
            lens.append(37 + (tot * 7919) % 964)
            tot += lens[-1]
        pos = torch.cat([torch.arange(n) for n in lens])[:M].to(torch.int32).to(dev)

    def launch():
        X = torch.cat([X0, torch.full((PAD_ROWS, N1), SENTINEL, device=dev)])
        part = torch.full((M + PAD_ROWS, nslab, 2), SENTINEL, device=dev)
        xh = torch.full((M + PAD_ROWS, N1), SENTINEL, device=dev).to(dt)
        stat = torch.full((M + PAD_ROWS, 2), SENTINEL, device=dev)
        out = torch.full((M + PAD_ROWS, nout), SENTINEL, device=dev).to(dt)
        produced, plan = C.c_int32(-1), (C.c_int32 * 10)()
        ptr = lambda t: None if t is None else t.data_ptr()
        _cabi.check(lib.opus_debug_gemm_ln(ctx, A.data_ptr(), dW1.data_ptr(), ptr(bias1), X.data_ptr(), part.data_ptr(), xh.data_ptr(),
                                           stat.data_ptr(), dW2.data_ptr(), ptr(c2_32), ptr(s32), out.data_ptr(), M, N1, K1, N2, epi,
                                           1 if rms else 0, eps, (rope_T if rope == "row" else 1026) if rope else 0, ptr(pos), C.byref(produced), plan, None))
        torch.cuda.synchronize()
        return X, part, xh, stat, out, produced.value, list(plan)

    X, part, xh, stat, out, produced, plan = launch()
    res = dict(shape=(M, N1, K1, N2), epi=epi, rms=rms, rope=rope, produced=produced, plan_producer=plan[:5], plan_consumer=plan[5:])
    if not produced:
        return res
    # ---- nothing behind row M was written
    sent16 = float(torch.tensor(SENTINEL).to(dt))
    res["pad_untouched"] = bool((X[M:] == SENTINEL).all() and (part[M:] == SENTINEL).all() and (stat[M:] == SENTINEL).all()
                                and (xh[M:].float() == sent16).all() and (out[M:].float() == sent16).all())
    X, part, xh, stat, out = X[:M], part[:M], xh[:M], stat[:M], out[:M]
    res["finite"] = bool(torch.isfinite(X).all() and torch.isfinite(stat).all() and torch.isfinite(out.float()).all())
    # ---- X against fp64, per class of rows (project rule for a GEMM output)
    Xref = R.producer_f64(X0.double(), A.double(), W1.double(), None if bias1 is None else bias1.double())
    d = (X.double() - Xref).abs()
    res["x_err"] = {CLASSES[i]: (float(d[m].max()), OUT_RULE[0] * float(Xref[m].abs().max()) + OUT_RULE[1]) for i, m in enumerate(masks)}
    del Xref, d
    # ---- the 16-bit hand-off is the rounded X, bit for bit
    res["xh_exact"] = bool(torch.equal(xh, X.to(dt)))
    # ---- partials against the fp64 sums of the X the kernel wrote; bound 4 x the fp32 emulation's worst error on the same data
    X64 = X.double()
    r1, r2 = R.partials_f64(X64)
    a1, a2 = R.partial_scales_f64(X64)
    e1 = float(((part[..., 0].double() - r1).abs() / (a1 + 1e-300)).max())
    e2 = float(((part[..., 1].double() - r2).abs() / (a2 + 1e-300)).max())
    w1, w2 = R.emulated_partial_error(X)
    res["part_err"] = dict(sum=(e1, 4 * w1), sumsq=(e2, 4 * w2), emulation=(w1, w2))
    del r1, r2, a1, a2
    # ---- (mu, rstd) against fp64 of the same X; bound per class 4 x the emulation's worst error there (grows as 1 + mu^2 / var)
    mu_r, rstd_r = R.stats_f64(X64, eps, rms)
    sig = ((X64 - X64.mean(1)[:, None]) ** 2).mean(1) ** 0.5
    em, er = R.stat_errors(stat[:, 0], stat[:, 1], mu_r, rstd_r, sig)
    wm, wr = R.emulated_stat_error(X, eps, rms)
    res["stat_err"] = {CLASSES[i]: dict(mu=(float(em[m].max()), 4 * float(wm[m].max())), rstd=(float(er[m].max()), 4 * float(wr[m].max())),
                                        mu_over_sigma=float((mu_r[m].abs() / sig[m].clamp_min(1e-30)).median()) if i < 5 else None)
                       for i, m in enumerate(masks)}
    if rms:
        res["rms_mu_zero"] = bool((stat[:, 0] == 0).all())
    # ---- the consumer against the kernel's own algebra in fp64 on the xh and stat the device produced (the tight one)
    cos = sin = None
    posl = None
    if rope:
        cos, sin = rope_table(1026, rope_theta, dev)
        posl = pos.long() if pos is not None else torch.arange(M, device=dev) % rope_T

    def finish(y):                                               # what follows the affine form: rounding + rotary
        if not rope:
            return y
        return R.rope_f64(R.round16(y, bf16), posl, N2 // 3, cos, sin, 0.125)

    s64 = None if s32 is None else s32.double()
    c64 = None if c2_32 is None else c2_32.double()
    alg = finish(R.consumer_fused_f64(xh.double(), stat[:, 0].double(), stat[:, 1].double(), Wf16, s64, c64, epi))
    got = out.double()
    f = BF16_FACTOR if bf16 else 1
    rule = ROPE_RULE * f * float(alg.abs().max()) if rope else f * OUT_RULE[0] * float(alg.abs().max()) + OUT_RULE[1]
    res["algebra_err"] = (float((got - alg).abs().max()), rule)
    # (row, column) of the largest difference: names the tile when the check fails
    res["algebra_argmax"] = [int(v) for v in divmod(int((got - alg).abs().argmax()), nout)]
    del alg
    # ---- accuracy against the exact norm followed by the GEMM, per class: the host model's fused-form error + the kernel rule
    exact = finish(R.consumer_exact_f64(X64, mu_r, rstd_r, Wf16, c64, epi))
    s1e, s2e = R.partials_f32(X)
    mu_e, rstd_e = R.finalize_f32(s1e, s2e, N1, eps, rms)
    model = finish(R.consumer_fused_f64(R.round16(X, bf16), mu_e.double(), rstd_e.double(), Wf16, s64, c64, epi))
    scale = float(exact.abs().max())
    derr, dmodel = (got - exact).abs(), (model - exact).abs()
    acc = {}
    for i, m in enumerate(masks):
        kernel_rule = (ROPE_RULE * f * scale) if rope else (f * OUT_RULE[0] * scale + OUT_RULE[1])
        acc[CLASSES[i]] = dict(fused=float(derr[m].max()) / scale, model=float(dmodel[m].max()) / scale,
                               bound=(float(dmodel[m].max()) + kernel_rule) / scale)
    del model, derr, dmodel
    # the stand-alone form on the same rows: the norm in fp32 (as rownorm_kernel: two-pass mean / variance), rounded to 16 bits,
    # through the plain GEMM with the same folded weight - measured, not asserted (the product's no_ln_fusion path)
    if standalone and not rope:
        x32 = X.float()
        if rms:
            xn = x32 * torch.rsqrt((x32 * x32).mean(1, keepdim=True) + eps)
        else:
            mu32 = x32.mean(1, keepdim=True)
            xn = (x32 - mu32) * torch.rsqrt(((x32 - mu32) ** 2).mean(1, keepdim=True) + eps)
        xn = xn.to(dt).contiguous()
        o2 = torch.empty(M, nout, dtype=dt, device=dev)
        _cabi.check(lib.opus_debug_gemm(ctx, xn.data_ptr(), dW2.data_ptr(), None if c2_32 is None else c2_32.data_ptr(), None, o2.data_ptr(),
                                        M, N2, N1, epi, 0, None))
        torch.cuda.synchronize()
        d2 = (o2.double() - exact).abs()
        for i, m in enumerate(masks):
            acc[CLASSES[i]]["standalone"] = float(d2[m].max()) / scale
        del d2, o2, xn
    res["accuracy"] = acc
    del exact, X64
    # ---- the same launch again: the same bits (the pair combine adds in arrival order; a + b is one fp32 number either way)
    same = True
    for _ in range(repeats):
        X2, part2, xh2, stat2, out2, _, plan2 = launch()
        same = same and plan2 == plan and torch.equal(X2[:M], X) and torch.equal(part2[:M], part) and torch.equal(xh2[:M], xh) \
            and torch.equal(stat2[:M], stat) and torch.equal(out2[:M], out)
    res["repeats_identical"] = same
    return res


def check_case(res, want_producer, want_consumer, want_parts=None):
    """Asserts one run_case() result.  want_*: NONE / PAIR / REDUCE as launch_pp reported them (not assumed from the shape)."""
    M, N1, K1, N2 = res["shape"]
    assert res["produced"] == 1, res
    pp, pc = res["plan_producer"], res["plan_consumer"]
    bm = -(-M // 256)
    assert pp[0] + pp[1] == bm * N1 // 256 and pc[0] + pc[1] == bm * N2 // 256, (pp, pc)        # gemm_pp_kernel ran both, every tile once
    assert pp[3] == want_producer and pc[3] == want_consumer, (pp, pc)
    for p in (pp, pc):
        assert (p[3] == NONE) == (p[1] == 0 and p[2] == 1) and (p[3] != PAIR or p[2] == 2) and (p[3] != REDUCE or 2 <= p[2] <= 8), p
    if want_parts is not None:
        assert pp[2] == want_parts, pp
    assert pp[4] == 0 and pc[4] == (1 if res["rope"] else 0), (pp, pc)
    assert res["pad_untouched"] and res["finite"], res
    for k, (err, bound) in res["x_err"].items():
        assert err <= bound, ("X", k, err, bound)
    assert res["xh_exact"]
    for k in ("sum", "sumsq"):
        err, bound = res["part_err"][k]
        assert err <= bound, ("partials", k, err, bound, res["part_err"]["emulation"])
    for k, v in res["stat_err"].items():
        for q in ("mu", "rstd"):
            assert v[q][0] <= v[q][1], ("stat", k, q, v)
    if res["rms"]:
        assert res["rms_mu_zero"]
    err, bound = res["algebra_err"]
    assert err <= bound, ("algebra", err, bound, res["algebra_argmax"])
    for k, v in res["accuracy"].items():
        assert v["fused"] <= v["bound"], ("accuracy", k, v)
    assert res["repeats_identical"]


def summarize(res):
    """run_case() result -> what the bf16 child hands to its parent: the plans, the flags, every check as error / bound
    (<= 1 passes; 0 / 0 counts as 0) and the accuracy figures by class."""
    ratio = lambda e, b: 0.0 if e == 0 else (e / b if b > 0 else float("inf"))
    out = dict(plan_producer=res["plan_producer"], plan_consumer=res["plan_consumer"], produced=res["produced"])
    out["flags_ok"] = bool(res["pad_untouched"] and res["finite"] and res["xh_exact"] and res["repeats_identical"])
    out["x"] = max(ratio(*v) for v in res["x_err"].values())
    out["partials"] = max(ratio(*res["part_err"]["sum"]), ratio(*res["part_err"]["sumsq"]))
    out["stat"] = max(max(ratio(*v["mu"]), ratio(*v["rstd"])) for v in res["stat_err"].values())
    out["algebra"] = ratio(*res["algebra_err"])
    out["accuracy"] = max(ratio(v["fused"], v["bound"]) for v in res["accuracy"].values())
    out["by_class"] = {k: {q: v[q] for q in ("fused", "standalone", "model") if q in v} for k, v in res["accuracy"].items()}
    return out
