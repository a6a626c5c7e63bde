"""Shared runner of tests/test_gpu_attn_forms.py and tests/bf16_attn_forms_check.py: launches attn_prefill_kernel through
opus_debug_attn_prefill as the product does (fused projection buffer, token strides of the whole row, padded / token-packed /
q_trim) and compares with tests/attn_forms_ref.py.  Returns observations; the callers assert the bounds."""
import ctypes as C

import torch

from opus_pllm_amd import _cabi
import attn_forms_ref as R


def sentinel_like(rows: int, cols: int, dtype, dev):
    return torch.full((rows, cols), R.SENTINEL, dtype=torch.int16, device=dev).view(dtype)


def bits(t):
    return t.view(torch.int16)


class knob_misc3:
    """Knob misc3 (swaps the launcher's choice of query tiles per wave) for the length of a `with`, restored whatever happens."""

    def __init__(self, value: int):
        self.value = value

    def __enter__(self):
        if self.value:
            _cabi.check(_cabi.lib().opus_debug_knob(None, b"misc3", self.value))

    def __exit__(self, *exc):
        if self.value:
            _cabi.check(_cabi.lib().opus_debug_knob(None, b"misc3", 0))


def launch(ctx, case: R.Case, d_qkv, d_out, *, trim=None, d_cu=None, d_kstart=None, d_kend=None, B=None, T=None, knob=None,
           overrides=None):
    """One opus_debug_attn_prefill call on the fused buffer of `case`.  Returns (return code, qt_used)."""
    cq, ck, cv = case.cols
    es = d_qkv.element_size()
    D = case.heads * case.hd
    a = dict(q_st=case.width, k_st=case.width, v_st=case.width, o_st=D, q_sb=case.T * case.width, k_sb=case.T * case.width,
             v_sb=case.T * case.width, o_sb=case.T * D, B=case.B if B is None else B, T=case.T if T is None else T, hd=case.hd,
             causal=case.causal)
    a.update(overrides or {})
    qt = C.c_int32(-1)
    ptr = lambda t: None if t is None else t.data_ptr()                # noqa: E731
    with knob_misc3(case.knob if knob is None else knob):
        rc = _cabi.lib().opus_debug_attn_prefill(
            ctx, d_qkv.data_ptr() + cq * es, d_qkv.data_ptr() + ck * es, d_qkv.data_ptr() + cv * es, d_out.data_ptr(), a["q_st"],
            a["k_st"], a["v_st"], a["o_st"], a["q_sb"], a["k_sb"], a["v_sb"], a["o_sb"], ptr(d_kstart), ptr(d_kend), ptr(d_cu), a["B"],
            a["T"], case.heads, case.group, a["hd"], a["causal"], case.trim if trim is None else trim, case.scale, C.byref(qt), None)
    return rc, qt.value


def run_family(dev, ctx, case: R.Case, family: str, dtype):
    lib = _cabi.lib()
    inp = R.make_inputs(case, family, dtype)
    ref = R.reference_case(case, inp)
    obs = {}
    if family == "peaked":
        obs["mass"] = R.peaked_mass(case, inp, ref)
        assert obs["mass"] >= R.MASS_MIN, (case.name, obs["mass"])       # the family's premise, before anything is compared
    D = case.heads * case.hd
    nrows = case.rows + R.GUARD_ROWS
    d_qkv = inp["qkv"].to(dev)
    dv = {k: None if inp[k] is None else inp[k].to(dev) for k in ("cu", "kstart", "kend")}
    args = dict(d_cu=dv["cu"], d_kstart=dv["kstart"], d_kend=dv["kend"])

    def run(**kw):
        out = sentinel_like(nrows, D, dtype, dev)
        rc, qt = launch(ctx, case, d_qkv, out, **{**args, **kw})
        if rc != 0:
            raise _cabi.OpusError(rc, lib.opus_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        return out.cpu(), qt

    o, obs["qt_used"] = run()
    o2, qt2 = run()
    obs["repeat_bitwise"] = bool(torch.equal(bits(o), bits(o2))) and qt2 == obs["qt_used"]
    obs["qkv_untouched"] = bool(torch.equal(bits(d_qkv.cpu()), bits(inp["qkv"])))
    sent = torch.full((D,), R.SENTINEL, dtype=torch.int16)
    obs["guard_rows_kept"] = bool((bits(o[case.rows:]) == sent).all())

    err, zero_ok, kept_ok, n_checked, n_zero = 0.0, True, True, 0, 0
    for b in range(case.B):
        out, computed, has_key, _ = ref[b]
        r0, n = case.row_start(b), case.row_len(b)
        ob = o[r0:r0 + n]
        chk = computed & has_key
        if bool(chk.any()):
            err = max(err, float((ob[chk].double().view(-1, case.heads, case.hd) - out[chk]).abs().max()))
        dark = computed & ~has_key
        zero_ok &= bool((ob[dark].float() == 0).all())
        kept_ok &= bool((bits(ob[~computed]) == sent).all())
        n_checked += int(chk.sum())
        n_zero += int(dark.sum())
    obs.update(err=err, dark_rows_zero=zero_ok, trimmed_rows_kept=kept_ok, rows_checked=n_checked, rows_dark=n_zero)

    if case.form == "packed":
        # every protein as a packed batch of one (its rows of the same buffer, the same QT): the same bits as inside the batch
        alone_ok, n_alone = True, 0
        for b in range(case.B):
            r0, n = case.row_start(b), case.row_len(b)
            if case.trim and n <= 2:
                continue                                                 # (no query: the entry refuses q_trim at T <= 2, as the path never launches it)
            cu1 = torch.tensor([r0, r0 + n], dtype=torch.int32, device=dev)
            oa, qta = run(d_cu=cu1, B=1, T=n, knob=0 if case.qt == R.qt_rule(1, case.heads, n, case.hd) else 1)
            q0, q1 = case.query_range(b)
            same = torch.equal(bits(oa[r0 + q0:r0 + q1]), bits(o[r0 + q0:r0 + q1]))
            rest = torch.cat([bits(oa[:r0 + q0]), bits(oa[r0 + q1:])])
            alone_ok &= bool(same) and qta == case.qt and bool((rest == sent).all())
            n_alone += 1
        obs.update(alone_bitwise=alone_ok, alone_runs=n_alone)
        if case.trim:
            full, qtf = run(trim=0)
            eq = qtf == case.qt
            for b in range(case.B):
                r0, n = case.row_start(b), case.row_len(b)
                eq &= bool(torch.equal(bits(full[r0 + 1:r0 + n - 1]), bits(o[r0 + 1:r0 + n - 1])))
            obs["trim_equals_full_bitwise"] = bool(eq)
    return obs


def run_case(dev, ctx, case: R.Case, dtype=None):
    dtype = dtype or _cabi.operand_dtype()
    return {f: run_family(dev, ctx, case, f, dtype) for f in ("random", "peaked")}


def failures(case: R.Case, obs, bound: float):
    """What of `obs` (run_case) breaks the rules of the form tests; empty = pass."""
    bad = []
    for fam, o in obs.items():
        if o["qt_used"] != case.qt:
            bad.append(f"{fam}: the launcher took QT {o['qt_used']}, the case expects {case.qt}")
        if not o["err"] <= bound:
            bad.append(f"{fam}: max |O - ref| = {o['err']:.3e} > {bound}")
        if o["rows_checked"] == 0:
            bad.append(f"{fam}: no row was compared")
        for flag in ("dark_rows_zero", "trimmed_rows_kept", "guard_rows_kept", "qkv_untouched", "repeat_bitwise", "alone_bitwise",
                     "trim_equals_full_bitwise"):
            if flag in o and not o[flag]:
                bad.append(f"{fam}: {flag} is false")
    return bad


def refusals(dev, ctx):
    """Calls the launcher or the entry must refuse without a launch: {name: (return code, qt_used, O untouched)}."""
    case = R.Case("refuse", "padded", 1, 16, 1, 1, 16, 1, lens=(16,))
    dt = _cabi.operand_dtype()
    d_qkv = torch.zeros(64, 64, dtype=dt, device=dev)
    cu = torch.tensor([0, 16], dtype=torch.int32, device=dev)
    tries = {
        "q_stride_not_multiple_of_8": dict(overrides=dict(q_st=case.width + 4)),
        "o_stride_not_multiple_of_4": dict(overrides=dict(o_st=18)),
        "k_offsets_reach_2^31": dict(overrides=dict(k_st=1 << 26)),           # 16 tokens x 2^26 elements x 2 bytes = 2^31
        "v_offsets_reach_2^31": dict(overrides=dict(v_st=1 << 26)),
        "head_dim_48": dict(overrides=dict(hd=48, q_st=144, k_st=144, v_st=144, o_st=48)),
        "causal_with_cu": dict(overrides=dict(causal=1), d_cu=cu),
        "q_trim_without_cu": dict(trim=1),
    }
    res = {}
    for name, kw in tries.items():
        out = sentinel_like(64, 64, dt, dev)
        rc, qt = launch(ctx, case, d_qkv, out, **kw)
        torch.cuda.synchronize()
        res[name] = (rc, qt, bool((bits(out) == R.SENTINEL).all().item()))
    return res
