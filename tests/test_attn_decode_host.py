"""CPU side of the decode-attention kernel tests (tests/test_gpu_attn_decode.py): the reference against torch's own attention,
the premises of the peaked and fused input families, the case table against the restated tiling and launcher rule, the layout
function, and the new entry's binding and first argument checks."""
import ctypes as C
import os

import pytest
import torch

from opus_pllm_amd import _cabi
import attn_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
NAME = "opus_debug_attn_decode_form"


@pytest.mark.parametrize("name", ["hd32_g3.random.L33.B7", "hd64_g4.random.L159.B7", "hd128_g8.fused.ks8.B64", "hd32_g2.peaked.L128.B7",
                                  "hd16_g1.random.L1.B7"])
def test_reference_matches_torch_sdpa(name):
    """`reference` against scaled_dot_product_attention in fp64 on an explicit boolean mask over slots kstart .. L, on the
    operands the reference itself rounds (rotated query and key, value), hidden slots zeroed."""
    case = R.CASE_BY_NAME[name]
    c, B, L = case.c, case.B, case.L
    dt = torch.float16
    inp = R.make_inputs(case, dt)
    O, kn, vn, P, amb = R.reference_case(case, inp, dt)
    proj = R.fused_projection(inp["slabs"], inp["ssq"], case.K, R.EPS, inp["bias"])[0] if case.family == "fused" else inp["qkv"]
    p = proj.to(dt).double()
    kstart = inp["kstart"].long()
    q = R.rope64(p[:, : c.nh * c.hd].view(B, c.nh, c.hd), L - kstart).to(dt).double()
    hidden = torch.arange(L + 1)[None, :] < kstart[:, None]
    K = torch.cat([inp["k_hist"].double(), kn.to(dt).double()[:, :, None]], 2)
    V = torch.cat([inp["v_hist"].double(), vn.double()[:, :, None]], 2)
    K = torch.where(hidden[:, None, :, None], torch.zeros_like(K), K).repeat_interleave(c.G, 1)
    V = torch.where(hidden[:, None, :, None], torch.zeros_like(V), V).repeat_interleave(c.G, 1)
    want = torch.nn.functional.scaled_dot_product_attention(q[:, :, None, :], K, V, attn_mask=~hidden[:, None, None, :])
    assert float((O - want.reshape(B, -1)).abs().max()) < 1e-12
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12
    assert float(P.masked_select(hidden[:, None, :].expand_as(P)).abs().sum()) == 0.0
    assert bool(torch.isnan(inp["k_hist"].float()).any()) == bool((kstart > 0).any())


@pytest.fixture(scope="module")
def peaked():
    cache = {}

    def get(dt):
        if dt not in cache:
            cache[dt] = {}
            for c in R.CASES:
                if c.family == "peaked":
                    inp = R.make_inputs(c, dt)
                    cache[dt][c.name] = (inp, R.reference_case(c, inp, dt))
        return cache[dt]
    return get


@DTYPES
def test_peaked_family_premises(peaked, dt):
    """Every query's reference mass on pi(b, h) is at least 0.99 in both operand types (so O = V[pi] up to rounding); pi aims
    only at visible slots and, over the queries of a case, reaches the first visible key, the last cached key, the new key, both
    sides of every 32-slot boundary in the visible range and a key of every wave's share; operands finite, |q| < 128."""
    worst = 1.0
    for c in R.CASES:
        if c.family != "peaked":
            continue
        inp, (O, kn, vn, P, amb) = peaked(dt)[c.name]
        mass = R.peaked_mass(c, inp, P)
        assert mass >= R.MASS_MIN, (c.name, mass)
        worst = min(worst, mass)
        pi = inp["pi"]
        ks = inp["kstart"].long()
        assert bool(((pi >= ks[:, None]) & (pi <= c.L)).all()), c.name
        hit = {k for b in range(c.B) for k, s in R.pi_targets(c, b) if bool((pi[b] == s).any())}
        assert hit == R.target_kinds(c), (c.name, R.target_kinds(c) - hit)
        assert {"kstart", "new"} <= hit and ("last_cached" in hit) and "wave_0" in hit
        q = inp["qkv"].float()
        assert bool(torch.isfinite(q).all()) and float(q.abs().max()) < 128, c.name
        assert float((O.view(c.B, c.c.nh, c.c.hd) - torch.cat([inp["v_hist"].double(), vn.double()[:, :, None]], 2)
                      .repeat_interleave(c.c.G, 1).nan_to_num(0.0).gather(2, pi[:, :, None, None].expand(-1, -1, 1, c.c.hd))[:, :, 0]).abs().max()) < 0.1
    print("smallest mass", dt, worst)


@DTYPES
def test_fused_family_ambiguous_share(dt):
    """At most 5 % of a fused case's projection elements lie within 2^-20 of their magnitude of a rounding boundary - a condition
    on the inputs: everywhere else the kernel's fp32 evaluation must round as fp64 does."""
    shares = {}
    for c in R.CASES:
        if c.family != "fused":
            continue
        inp = R.make_inputs(c, dt)
        x, mag = R.fused_projection(inp["slabs"], inp["ssq"], c.K, R.EPS, inp["bias"])
        amb = R.ambiguous(x, mag, dt)
        shares[c.name] = float(amb.float().mean())
        assert shares[c.name] <= 0.05, (c.name, shares[c.name])
        assert inp["slabs"].dtype == torch.float32 and inp["ssq"].shape == (c.B, c.nblk)
        assert float(inp["ssq"].min()) >= 50 and float(inp["ssq"].max()) < 250 and (inp["bias"] is not None) == bool(c.bias)
    print(dt, min(shares.values()), max(shares.values()))


@DTYPES
def test_value_check_against_an_fp32_evaluation(dt):
    """The rule the appended value is held to on the GPU, tried on a plain fp32 evaluation of (sum of slabs) * rstd + bias in
    torch: it equals the fp64 rounding off the ambiguous set and is the rounding of a value within 2^-20 mag everywhere; the
    neighbours of the fp64 rounding pass nowhere off the ambiguous set (so a kernel one step off there fails).  More than one
    step off happens, on sums that cancelled to ~1e-4: that is why the rule is the interval, not a step count."""
    beyond = 0
    for c in R.CASES:
        if c.family != "fused":
            continue
        inp = R.make_inputs(c, dt)
        x, mag = R.fused_projection(inp["slabs"], inp["ssq"], c.K, R.EPS, inp["bias"])
        amb, r = R.ambiguous(x, mag, dt), x.to(dt)
        v = torch.zeros_like(inp["slabs"][0])
        for k in range(c.ks):
            v = v + inp["slabs"][k]
        v = v * torch.rsqrt(inp["ssq"].sum(1) / c.K + R.EPS)[:, None]
        v = (v + inp["bias"] if c.bias else v).to(dt)
        assert bool(R.rounds_from_nearby(v, x, mag).all()), c.name
        assert bool((v.view(torch.int16) == r.view(torch.int16))[~amb].all()), c.name
        assert bool(R.rounds_from_nearby(r, x, mag).all())
        for nb in R._neighbours(r):
            assert not bool((R.rounds_from_nearby(nb.to(dt), x, mag) & ~amb).any()), c.name
        far = ~R.one_ulp_apart(v, r)
        assert float(x[far].abs().max() if far.any() else 0.0) < 1e-2
        beyond += int(far.sum())
    print(dt, "more than one step off:", beyond)


@DTYPES
def test_ambiguous_marks_boundaries_only(dt):
    """A value on the midpoint of two neighbours is ambiguous, one a quarter step away or on a representable value is not; the
    neighbours are the adjacent representable values, across zero and across a power of two."""
    r = torch.tensor([1.0, 1.5, -2.0, 0.3330078125, 0.0, -0.75], dtype=torch.float64).to(dt)
    up, dn = R._neighbours(r)
    rd = r.double()
    assert bool((up > rd).all()) and bool((dn < rd).all())
    assert bool((up.to(dt).double() == up).all()) and bool((dn.to(dt).double() == dn).all())
    for a, b in ((rd, up), (dn, rd)):                      # nothing representable strictly between
        mid = (a + b) / 2
        assert bool(((mid.to(dt).double() == a) | (mid.to(dt).double() == b)).all())
    mag = rd.abs()                                         # (zero: only the boundary itself is ambiguous)
    assert bool(R.ambiguous((rd + up) / 2, mag, dt).all()) and bool(R.ambiguous((rd + dn) / 2, mag, dt).all())
    assert not bool(R.ambiguous(rd, mag, dt).any()) and not bool(R.ambiguous(rd + (up - rd) / 4, mag, dt)[[0, 1, 2, 3, 5]].any())
    assert bool(R.one_ulp_apart(up.to(dt), r).all()) and bool(R.one_ulp_apart(r, r).all())
    assert not bool(R.one_ulp_apart((up + (up - rd)).to(dt), r)[[0, 1, 2, 3, 5]].any())


def test_case_table_reaches_every_cell():
    reached = set()
    for c in R.CASES:
        cells = R.geometry_cells(c)
        assert cells <= set(R.REQUIRED), (c.name, cells - set(R.REQUIRED))
        reached |= cells
    assert reached == set(R.REQUIRED), sorted(set(R.REQUIRED) - reached)
    assert len(set(R.REQUIRED)) == len(R.REQUIRED) == 16 + 20 + 17
    # per context: every tiling cell its own cases can reach, so that no instance leans on another's cases
    for ctx in R.CONTEXTS:
        mine = set().union(*(R.geometry_cells(c) for c in R.cases_of(ctx.name)))
        assert {x for x in R.TILING_CELLS if not x.startswith(("ne.", "group_3"))} <= mine, ctx.name
    for name in R.FUSED_CONTEXTS:
        for B in (7, 64):
            mine = set().union(*(R.geometry_cells(c) for c in R.cases_of(name) if c.family == "fused" and c.B == B))
            assert set(R.FUSED_CELLS) - {"form.unfused"} <= mine, (name, B)


def test_case_table_matches_the_issue_and_the_rule():
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)
    assert {(c.hd, c.G) for c in R.CONTEXTS if c.nkv == 4 and c.G != 3} == {(h, g) for h in (16, 32, 64, 128) for g in (1, 2, 4, 8)}
    assert [(c.hd, c.nh, c.nkv) for c in R.CONTEXTS if c.G == 3] == [(16, 12, 4), (32, 6, 2)]
    assert all(c.nh * c.hd % 64 == 0 for c in R.CONTEXTS)                  # (what opus_ctx_create asks of every context)
    assert R.CTX_CAP == R.MAX_PROMPT + R.MAX_NEW == 160
    for dt in (torch.float16, torch.bfloat16):
        assert bool(torch.isnan(R.nan_like((3,), dt).float()).all())
        assert bool(torch.isfinite(torch.tensor([R.SENTINEL], dtype=torch.int16).view(dt).float()).all())
    seen = set()
    for c in R.CASES:
        assert c.gp == R.gp_rule(c.B, c.c.nh, c.c.nkv) and c.B in (7, 64), c.name
        assert c.gp == (c.c.G if c.B == 64 and c.c.G in (2, 4, 8) and c.c.nkv == 4 else 1), c.name
        assert 1 <= c.T0 <= R.MAX_PROMPT and 0 <= c.step < R.MAX_NEW and c.L < R.CTX_CAP
        assert all(0 <= k <= c.T0 - 1 for k in c.kstart)
        seen.add((c.c.hd, c.gp))
        if c.family == "fused":
            assert c.ctx in R.FUSED_CONTEXTS and c.L in (33, 159) and 1 <= c.ks <= 8 and c.nblk in (1, 16, 65, 300) and c.K == 256 * c.nblk
            assert 4 < c.B <= 64 and c.c.nh * c.c.hd % 256 == 0 or c.ctx == "hd16_g2"        # (the product's own gate; hd16_g2 is narrower)
    assert seen == {(h, g) for h in (16, 32, 64, 128) for g in (1, 2, 4, 8)}                  # all 16 instances
    assert R.gp_rule(64, 12, 4) == 1 and 64 * 4 >= R.GROUP_MIN > 64 * 2 and R.gp_rule(64, 6, 2) == 1 and R.gp_rule(63, 32, 4) == 1 and R.gp_rule(64, 32, 4) == 8
    assert R.ne_of(128, 8) == 3 and [R.ne_of(h, g) for h, g in ((128, 4), (64, 8), (128, 2), (16, 8))] == [2, 2, 1, 1]
    for c in R.CONTEXTS:
        plain = [x for x in R.cases_of(c.name) if x.family != "fused"]
        assert {x.L for x in plain} == {1, 31, 32, 33, 63, 64, 96, 127, 128, 159}
        assert {(x.L, x.B, x.family) for x in plain} == {(L, B, f) for L in {x.L for x in plain} for B in (7, 64) for f in ("random", "peaked")}
    ks = {k for c in R.CASES for k in c.kstart}
    assert {0, 1, 31, 32, 33, 65, 95} <= ks                     # (a prompt row has a token: kstart <= T0 - 1 <= 95)
    bf = [R.CASE_BY_NAME[n] for n in R.BF16_CASES]
    assert (bf[0].c.hd, bf[0].gp) == (16, 4) and (bf[1].c.hd, bf[1].gp, bf[1].family, bf[1].bias) == (128, 8, "fused", 1)
    assert bf[2].gp == 1 and bf[2].L < 128


@pytest.mark.parametrize("B,K", [(1, 64), (7, 128), (16, 64), (17, 192), (64, 512), (64, 4096)])
def test_tiled_off_is_a_bijection(B, K):
    rows = R.tiled_rows(B)
    off = R.tiled_off(torch.arange(rows)[:, None], torch.arange(K)[None, :], K).reshape(-1)
    assert sorted(off.tolist()) == list(range(rows * K))
    assert R.tiled_off(0, 0, K) == 0 and R.tiled_off(1, 0, K) == 8 and R.tiled_off(0, 8, K) == 128 and R.tiled_off(0, 32, K) == 512
    flat = torch.arange(rows * K, dtype=torch.int32)
    assert torch.equal(R.untile(flat, rows, K).reshape(-1).long(), off)
    src = open(os.path.join(ROOT, "opus-pllm_amd", "csrc", "common.h")).read()
    assert "((int64_t)(row >> 4) * (K >> 6) + (k >> 6)) * 1024 + ((k & 63) >> 5) * 512 + ((((k & 31) >> 3) << 4) + (row & 15)) * 8 + (k & 7)" in src


def test_signature_is_bound():
    res, args = _cabi.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 23 and args[-2] == C.POINTER(C.c_int32) and args[7] is C.c_float
    header = open(os.path.join(ROOT, "include", "opus_pllm.h")).read()
    assert NAME + "(" in header and "opus_debug_attn_decode(" in header and "#define OPUS_ABI_VERSION 10" in header
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read() and NAME in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "attn_decode_group(" in open(os.path.join(ROOT, "opus-pllm_amd", "csrc", "attn_decode.hip")).read()


@pytest.mark.parametrize("so", ["libopus_pllm.so", "libopus_pllm_bf16.so"])
def test_symbol_is_exported(so):
    lib = C.CDLL(os.path.join(ROOT, "opus-pllm_amd", "lib", so))
    assert getattr(lib, NAME) is not None and getattr(lib, "opus_debug_attn_decode") is not None
    assert lib.opus_abi_version() == 10


def test_first_argument_checks_return_before_any_device_call():
    """A null context is refused first (-1, gp_used 0).  With a context that is only a non-null address, the checks that come
    before the context is read are reached: a null d_kstart / d_out / gp_used, and both or neither of d_qkv / d_slabs."""
    lib = _cabi.lib()
    gp = C.c_int32(7)
    one = C.c_int64(0)
    p = C.addressof(one)

    def call(ctx=None, qkv=p, slabs=None, kstart=p, out=p, gpp=None):
        return lib.opus_debug_attn_decode_form(ctx, qkv, slabs, 1, p, 1, 256, 1e-5, None, p, p, kstart, 1, 4, 0, 0, out, None, None, None, None,
                                               C.byref(gp) if gpp is None else gpp, None)

    assert call() == -1 and gp.value == 0 and b"null" in lib.opus_last_error()
    assert lib.opus_debug_attn_decode(None, p, p, p, p, 1, 4, 0, p, None, None, None) == -1
    fake = C.c_int64(0)
    ctx = C.addressof(fake)                        # never dereferenced: every call below fails an earlier check
    for kw in (dict(kstart=None), dict(out=None), dict(qkv=p, slabs=p), dict(qkv=None, slabs=None)):
        gp.value = 7
        assert call(ctx=ctx, **kw) == -1 and gp.value == 0, kw
    assert call(ctx=ctx, gpp=C.POINTER(C.c_int32)()) == -1
