"""Shared runner of tests/test_gpu_attn_decode.py and tests/bf16_attn_decode_check.py: launches attn_decode_kernel through
opus_debug_attn_decode_form in every form the decode step takes (finished projections or raw slabs + sums of squares + bias;
row-major or fragment-ordered output) and compares with tests/attn_decode_ref.py.  Returns observations; the callers assert
the bounds."""
import ctypes as C

import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi
import attn_decode_ref as R


class RawCtx:
    """A context without weights: the kernel-level entry points need the workspace and the KV cache only."""

    def __init__(self, c: R.Ctx, dev):
        self.c, self.dev, self.lib, self.ctx = c, dev, _cabi.lib(), C.c_void_p()
        cc = _cabi.CConfig.from_config(opa.OpusConfig(**c.config_kwargs()).validate())
        _cabi.check(self.lib.opus_ctx_create(C.byref(cc), dev.index or 0, C.byref(self.ctx)))

    def close(self):
        if self.ctx.value:
            self.lib.opus_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()


def bits(t):
    return t.view(torch.int16)


def _ptr(t):
    return None if t is None else t.data_ptr()


def launch(r: RawCtx, dtype, d, B, T0, step, *, out_tiled=0, want_cache=False, ks=None, nblk=None, K=None, overrides=None):
    """One opus_debug_attn_decode_form call on device tensors d (qkv or slabs / ssq / bias, k_hist, v_hist, kstart).  Returns a
    dict: rc, gp, out [B, D] (host, row-major whatever the launch wrote), clean (everything of O behind row B - 1 kept its
    sentinel), k_new / v_new, and with want_cache the whole layer-0 cache."""
    c, dev = r.c, r.dev
    D = c.nh * c.hd
    fused = d.get("slabs") is not None
    rows = (R.tiled_rows(B) + 16) if out_tiled else (B + R.GUARD_ROWS)
    out = torch.full((rows, D), R.SENTINEL, dtype=torch.int16, device=dev).view(dtype)
    k_new = torch.zeros(B, c.nkv, c.hd, dtype=dtype, device=dev)
    v_new = torch.zeros_like(k_new)
    kc = vc = None
    if want_cache:
        kc = torch.zeros(B, c.nkv, R.CTX_CAP, c.hd, dtype=dtype, device=dev)
        vc = torch.zeros_like(kc)
    a = dict(qkv=_ptr(d.get("qkv")), slabs=_ptr(d.get("slabs")), ks=(ks if ks is not None else d["slabs"].shape[0]) if fused else 0,
             ssq=_ptr(d.get("ssq")), nblk=(nblk if nblk is not None else d["ssq"].shape[1]) if fused else 0,
             K=(K if K is not None else 256 * d["ssq"].shape[1]) if fused else 0, bias=_ptr(d.get("bias")), k_hist=_ptr(d["k_hist"]),
             v_hist=_ptr(d["v_hist"]), kstart=_ptr(d["kstart"]), B=B, T0=T0, step=step, out_tiled=out_tiled, out=out.data_ptr())
    a.update(overrides or {})
    gp = C.c_int32(7)
    rc = r.lib.opus_debug_attn_decode_form(r.ctx, a["qkv"], a["slabs"], a["ks"], a["ssq"], a["nblk"], a["K"], R.EPS, a["bias"], a["k_hist"],
                                           a["v_hist"], a["kstart"], a["B"], a["T0"], a["step"], a["out_tiled"], a["out"], k_new.data_ptr(),
                                           v_new.data_ptr(), _ptr(kc), _ptr(vc), C.byref(gp), None)
    torch.cuda.synchronize()
    o = out.cpu()
    res = dict(rc=rc, gp=gp.value, raw=o)
    if rc != 0:
        return res
    sent = torch.tensor(R.SENTINEL, dtype=torch.int16)
    if out_tiled:
        n = R.tiled_rows(B)
        rm = R.untile(o.reshape(-1)[: n * D], n, D)
        res["clean"] = bool((bits(rm[B:]) == sent).all()) and bool((bits(o.reshape(-1)[n * D:]) == sent).all())
        res["out"] = rm[:B]
    else:
        res["clean"] = bool((bits(o[B:]) == sent).all())
        res["out"] = o[:B]
    res.update(k_new=k_new.cpu(), v_new=v_new.cpu())
    if want_cache:
        res.update(k_cache=kc.cpu(), v_cache=vc.cpu())
    return res


def _need(res, what):
    if res["rc"] != 0:
        raise _cabi.OpusError(res["rc"], what + ": " + _cabi.lib().opus_last_error().decode("utf-8", "replace"))
    return res


DEVICE_KEYS = ("qkv", "slabs", "ssq", "bias", "k_hist", "v_hist", "kstart")


def run_case(r: RawCtx, case: R.Case, dtype=None):
    dtype = dtype or _cabi.operand_dtype()
    c, dev = r.c, r.dev
    B, L, T0, step, D = case.B, case.L, case.T0, case.step, c.nh * c.hd
    inp = R.make_inputs(case, dtype)
    O, kn, vn, P, amb = R.reference_case(case, inp, dtype)
    obs = {}
    if case.family == "peaked":
        obs["mass"] = R.peaked_mass(case, inp, P)
        assert obs["mass"] >= R.MASS_MIN, (case.name, obs["mass"])       # the family's premise, before anything is compared
    primary = case.out_tiled if case.family == "fused" else 0

    # every slot of the rows' cache <- NaN, through a launch of its own (slot 159 is the kernel's own NaN)
    p = R.poison_inputs(c, B, dtype)
    pd = {k: p[k].to(dev) for k in ("qkv", "k_hist", "v_hist", "kstart")}
    base = _need(launch(r, dtype, pd, B, p["T0"], p["step"], want_cache=True), "poison launch")
    obs["poisoned"] = bool(torch.isnan(base["k_cache"].float()).all()) and bool(torch.isnan(base["v_cache"].float()).all())

    d = {k: inp[k].to(dev) for k in DEVICE_KEYS if inp.get(k) is not None}
    a = _need(launch(r, dtype, d, B, T0, step, out_tiled=primary, want_cache=True), case.name)
    b2 = _need(launch(r, dtype, d, B, T0, step, out_tiled=primary, want_cache=True), case.name)
    obs["gp_used"] = a["gp"]
    obs["repeat_bitwise"] = all(torch.equal(bits(a[k]), bits(b2[k])) for k in ("out", "k_new", "v_new", "k_cache", "v_cache")) and b2["gp"] == a["gp"]
    obs["guard_rows_kept"] = a["clean"] and b2["clean"]
    o2 = _need(launch(r, dtype, d, B, T0, step, out_tiled=1 - primary), case.name)
    obs["tiled_equals_row_major"] = bool(torch.equal(bits(o2["out"]), bits(a["out"]))) and o2["clean"] and o2["gp"] == a["gp"]
    obs["inputs_untouched"] = all(torch.equal(d[k].cpu().view(torch.uint8).reshape(-1), inp[k].contiguous().view(torch.uint8).reshape(-1)) for k in d)

    out = a["out"]
    if case.family == "fused":
        # the appended value: the rounding of the fp64 projection wherever fp32 can decide it; elsewhere a rounding of some value
        # inside the fp32 evaluation's error (one step off at most, but for sums that cancelled to almost nothing)
        x, mag = R.fused_projection(inp["slabs"], inp["ssq"], case.K, R.EPS, inp["bias"])
        vcol = (c.nh + c.nkv) * c.hd
        av = amb[:, vcol:].reshape(B, c.nkv, c.hd)
        xv, magv = (t[:, vcol:].reshape(B, c.nkv, c.hd) for t in (x, mag))
        same = bits(a["v_new"]) == bits(vn)
        near = R.one_ulp_apart(a["v_new"], vn)
        obs["v_exact_off_ambiguous"] = bool(same[~av].all())
        obs["v_in_rounding_interval"] = bool(R.rounds_from_nearby(a["v_new"], xv, magv).all())
        obs["ambiguous"] = int(amb.sum())
        obs["ambiguous_v_differ"] = int((~same[av]).sum())
        obs["ambiguous_v_beyond_one_step"] = int((~near).sum())
        # O against fp64 with the appended value the launch chose on the ambiguous set (either rounding is a right answer there,
        # and a value of 4 .. 8 that moves by one step moves O by up to 3.9e-3 when the new key holds the mass)
        O = R.reference_case(case, inp, dtype, v_new=torch.where(av, a["v_new"], vn))[0]
    else:
        obs["v_exact"] = bool(torch.equal(bits(a["v_new"]), bits(vn)))
    obs["finite"] = bool(torch.isfinite(out.float()).all())
    obs["err"] = float((out.double() - O).abs().max())
    obs["k_rel"] = float((a["k_new"].double() - kn).abs().max() / kn.abs().max())

    # the cache afterwards: slots < L are the history bit for bit (NaN patterns of hidden slots included), slot L is what the
    # launch reported as k_new / v_new, every later slot keeps what the poison launch left
    ok = True
    for name, hist, new in (("k_cache", inp["k_hist"], a["k_new"]), ("v_cache", inp["v_hist"], a["v_new"])):
        want = bits(base[name]).clone()
        want[:, :, :L] = bits(hist)
        want[:, :, L] = bits(new)
        ok &= bool(torch.equal(bits(a[name]), want))
    obs["cache_one_slot_written"] = ok

    if B == 7:
        alone = True
        for b in range(B):
            d1 = {k: (v if k == "bias" else v[:, b:b + 1].contiguous() if k == "slabs" else v[b:b + 1].contiguous()) for k, v in d.items()}
            o1 = _need(launch(r, dtype, d1, 1, T0, step, out_tiled=primary), case.name + " alone")
            alone &= bool(torch.equal(bits(o1["out"][0]), bits(out[b]))) and o1["gp"] == 1 and o1["clean"]
        obs["alone_bitwise"] = alone
    return obs


FLAGS = ("poisoned", "repeat_bitwise", "guard_rows_kept", "tiled_equals_row_major", "inputs_untouched", "finite", "v_exact",
         "v_exact_off_ambiguous", "v_in_rounding_interval", "cache_one_slot_written", "alone_bitwise")
K_REL = 2e-3               # tests/test_gpu_longctx.py: the appended key within 2e-3 max |ref| (four half-steps of fp16)
K_REL_BF16 = 1.6e-2        # the same rule with bf16's three fewer mantissa bits (x 8), as the bf16 build's GEMM rule


def failures(case: R.Case, obs, bound: float, k_rel: float = K_REL):
    """What of `obs` (run_case) breaks the rules of the decode-attention tests; empty = pass."""
    bad = []
    if obs["gp_used"] != case.gp:
        bad.append(f"the launcher took GP {obs['gp_used']}, the case expects {case.gp}")
    if not obs["err"] <= bound:
        bad.append(f"max |O - ref| = {obs['err']:.3e} > {bound}")
    if not obs["k_rel"] <= k_rel:
        bad.append(f"appended key off by {obs['k_rel']:.3e} of max |ref| > {k_rel}")
    bad += [f"{f} is false" for f in FLAGS if f in obs and not obs[f]]
    need = {"alone_bitwise"} if case.B == 7 else set()
    need |= {"tiled_equals_row_major"}
    need |= {"v_exact_off_ambiguous", "v_in_rounding_interval"} if case.family == "fused" else {"v_exact"}
    bad += [f"{f} was not checked" for f in sorted(need) if f not in obs]
    return bad


def summary(obs):
    return {k: obs[k] for k in ("err", "gp_used", "k_rel", "mass", "ambiguous", "ambiguous_v_differ", "ambiguous_v_beyond_one_step") if k in obs}


def refusals(r: RawCtx, dtype=None):
    """Calls the entry must refuse before any device call: {name: (return code, expected code, gp_used, O untouched)}.  (The
    entry's refusal of out_tiled with heads x head_dim off a multiple of 64 cannot be reached: no such context can be created.)"""
    dtype = dtype or _cabi.operand_dtype()
    c, dev = r.c, r.dev
    B, T0 = 5, 8
    z16 = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)                # noqa: E731
    plain = dict(qkv=z16(B, c.width), k_hist=z16(B, c.nkv, T0, c.hd), v_hist=z16(B, c.nkv, T0, c.hd),
                 kstart=torch.zeros(B, dtype=torch.int32, device=dev))
    fused = dict(plain, qkv=None, slabs=torch.zeros(2, B, c.width, device=dev), ssq=torch.ones(B, 3, device=dev))
    some = plain["qkv"].data_ptr()
    tries = {
        "null_out": (plain, {}, dict(out=None), -1),
        "null_kstart": (plain, {}, dict(kstart=None), -1),
        "null_history": (plain, {}, dict(k_hist=None), -1),
        "qkv_and_slabs": (fused, {}, dict(qkv=some), -1),
        "neither_qkv_nor_slabs": (plain, {}, dict(qkv=None), -1),
        "B_0": (plain, {}, dict(B=0), -2),
        "B_past_max_batch": (plain, {}, dict(B=R.MAX_BATCH + 1), -2),
        "T0_0": (plain, {}, dict(T0=0), -2),
        "T0_past_max_prompt": (plain, {}, dict(T0=R.MAX_PROMPT + 1), -2),
        "step_negative": (plain, {}, dict(step=-1), -2),
        "step_past_budget": (plain, {}, dict(step=R.MAX_NEW), -2),
        "ks_0": (fused, dict(ks=0), {}, -2),
        "ks_9": (fused, dict(ks=9), {}, -2),
        "row_nblk_0": (fused, dict(nblk=0), {}, -2),
        "slabs_without_row_ssq": (fused, {}, dict(ssq=None), -2),
    }
    res = {}
    for name, (d, kw, ov, want) in tries.items():
        o = launch(r, dtype, d, B, T0, 0, overrides=ov, **kw)
        res[name] = (o["rc"], want, o["gp"], bool((bits(o["raw"]) == R.SENTINEL).all()))
    return res
