"""Reference, inputs and case table of the decode-attention kernel tests (tests/test_attn_decode_host.py on the CPU,
tests/test_gpu_attn_decode.py on the GPU).  Plain torch on the CPU; nothing here touches the library.

attn_decode_kernel has 16 instances (head_dim 16 / 32 / 64 / 128 x GP = 1 / 2 / 4 / 8 query heads per workgroup), walks the
cache in 32-slot tiles dealt to four waves, and takes its input either as finished projections or as raw split-K slabs that it
sums, scales by the RMSNorm row factor, biases and rounds itself.  This module holds
  * `CONTEXTS`: one library context per (head_dim, group) plus two with a group of 3 (no grouped instance);
  * `CASES`: per context the launches, each with the GP the launcher must take;
  * three input families: `random`, `peaked` (query (b, h) is a multiple of key pi(b, h), so O = V[pi] up to rounding and a
    wrong key, V row, wave or tile is an O(1) error) and `fused` (slabs, sums of squares, bias);
  * `reference`: fp64 rotary + softmax over slots kstart .. L on the operands rounded as the kernel rounds them;
  * `ambiguous`: the elements of a fused projection that sit too close to a rounding boundary for fp32 to decide;
  * `geometry_cells`: a restatement of the kernel's tiling that lists which situations a case reaches, `REQUIRED` those the table
    must reach.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import torch

from attn_forms_ref import ALPHA as FORMS_ALPHA, MASS_MIN

TILE = 32                                 # cache slots per key tile
WAVES = 4
CTX_CAP = 160                             # max_prompt + max_new_tokens: five tiles, wave 0 gets a second one
MAX_PROMPT, MAX_NEW, MAX_BATCH = 96, 64, 64
THETA = 500000.0
GROUP_MIN = 256                           # the launcher's threshold: grouped workgroups from B * kv heads >= 256
SENTINEL = 0x7B2D                         # 16-bit pattern O is pre-filled with (a finite value in fp16 and in bf16)
NAN_BITS = 0x7FD5                         # a NaN in fp16 and in bf16: what hidden and never-written cache slots hold
GUARD_ROWS = 2                            # rows behind the last row of a row-major O (a tiled O has 16 more)
EPS = 1e-5
ALPHA = dict(FORMS_ALPHA)                 # peaked family: q = ALPHA k (see attn_forms_ref.py; the hd 16 value is already raised)
LENGTHS = ((1, 0), (31, 0), (30, 2), (33, 0), (40, 23), (64, 0), (96, 0), (96, 31), (65, 63), (96, 63))     # (T0, step)
KS_CHOICES = 8                            # kstart patterns a row cycles through (kstart_of)


@dataclass(frozen=True)
class Ctx:
    name: str
    hd: int
    nh: int
    nkv: int

    @property
    def G(self) -> int:
        return self.nh // self.nkv

    @property
    def width(self) -> int:
        return (self.nh + 2 * self.nkv) * self.hd

    def config_kwargs(self) -> dict:
        return dict(enc_layers=1, enc_dim=64, enc_heads=4, enc_ffn=64, proj_dim=64, dec_layers=1, dec_dim=64, dec_heads=self.nh,
                    dec_kv_heads=self.nkv, dec_head_dim=self.hd, dec_ffn=64, dec_vocab=64, dec_rope_theta=THETA, max_batch=MAX_BATCH,
                    max_enc_tokens=8, max_prompt=MAX_PROMPT, max_new_tokens=MAX_NEW)


CONTEXTS = [Ctx(f"hd{hd}_g{G}", hd, 4 * G, 4) for hd in (16, 32, 64, 128) for G in (1, 2, 4, 8)]
# a group of 3 has no grouped instance: per-head workgroups at every batch, one of three appends to the cache.  The first
# crosses the threshold at batch 64 (4 kv heads) and takes the launcher's fall-back, the second (6 heads, 2 kv heads) stays below.
# (A context needs heads x head_dim to be a multiple of 64 - the out-projection's reduction dim -, so 6 heads come with head_dim 32.)
CONTEXTS += [Ctx("hd16_g3", 16, 12, 4), Ctx("hd32_g3", 32, 6, 2)]
CTX_BY_NAME = {c.name: c for c in CONTEXTS}
FUSED_CONTEXTS = ("hd16_g2", "hd64_g4", "hd128_g8")


def gp_rule(B: int, nh: int, nkv: int) -> int:
    """attn_decode_group in csrc/attn_decode.hip."""
    G = nh // nkv
    return G if G in (2, 4, 8) and B * nkv >= GROUP_MIN else 1


@dataclass(frozen=True)
class Case:
    name: str
    ctx: str
    family: str                           # "random" | "peaked" | "fused"
    B: int
    T0: int
    step: int
    gp: int                               # query heads per workgroup the launcher must take
    rot: int = 0                          # which kstart pattern row 0 starts with
    ks: int = 0                           # fused: number of slabs
    nblk: int = 0                         # fused: blocks of the rows' sums of squares
    bias: int = 0
    out_tiled: int = 0                    # layout of the launch that is compared with fp64 (the other one must equal it)
    seed: int = 0

    @property
    def c(self) -> Ctx:
        return CTX_BY_NAME[self.ctx]

    @property
    def L(self) -> int:
        return self.T0 + self.step

    @property
    def K(self) -> int:
        return 256 * self.nblk

    def kstart_of(self, b: int) -> int:
        L = self.L
        choice = (0, 1, 31, 32, 33, 65, self.T0 - 1, L // TILE * TILE)[(b + self.rot) % KS_CHOICES]
        return min(choice, self.T0 - 1)

    @property
    def kstart(self) -> Tuple[int, ...]:
        return tuple(self.kstart_of(b) for b in range(self.B))


def _cases():
    out, seed = [], 1000
    for c in CONTEXTS:
        for i, (T0, step) in enumerate(LENGTHS):
            for B in (7, 64):
                for fam in ("random", "peaked"):
                    seed += 1
                    out.append(Case(f"{c.name}.{fam}.L{T0 + step}.B{B}", c.name, fam, B, T0, step, gp_rule(B, c.nh, c.nkv),
                                    rot=i + (3 if B == 64 else 0) + (fam == "peaked"), seed=seed))
        if c.name in FUSED_CONTEXTS:
            for B in (7, 64):
                for i in range(8):
                    seed += 1
                    T0, step = ((33, 0), (96, 63))[i & 1]
                    big = B == 64
                    out.append(Case(f"{c.name}.fused.ks{i + 1}.B{B}", c.name, "fused", B, T0, step, gp_rule(B, c.nh, c.nkv), rot=i + 2 * big,
                                    ks=i + 1, nblk=(1, 16, 65, 300)[(i + (i >> 2) + big) % 4], bias=((i >> 1) ^ i ^ big) & 1,
                                    out_tiled=((i >> 2) ^ big) & 1, seed=seed))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
BF16_CASES = ("hd16_g4.random.L159.B64", "hd128_g8.fused.ks8.B64", "hd64_g2.peaked.L33.B7")     # grouped hd 16, <128, 8> fused with bias, short per-head


def cases_of(ctx_name: str):
    return [c for c in CASES if c.ctx == ctx_name]


# ------------------------------------------------------------------------------------------------ layout
def tiled_off(row, k, K):
    """common.h tiled_off: offset of element (row, k) of a fragment-ordered [rows, K] 16-bit matrix (16-row x 64-k blocks of
    1024 elements in MFMA operand order).  Works on ints and on integer tensors."""
    return ((row >> 4) * (K >> 6) + (k >> 6)) * 1024 + ((k & 63) >> 5) * 512 + ((((k & 31) >> 3) << 4) + (row & 15)) * 8 + (k & 7)


def tiled_rows(B: int) -> int:
    return 16 * (-(-B // 16))


def untile(flat: torch.Tensor, rows: int, K: int) -> torch.Tensor:
    """[rows, K] row-major view of a fragment-ordered buffer (any 16-bit dtype)."""
    r = torch.arange(rows)[:, None]
    k = torch.arange(K)[None, :]
    return flat.reshape(-1)[tiled_off(r, k, K)]


# ------------------------------------------------------------------------------------------------ reference
def rope64(x, pos, theta=THETA):
    """x [B, h, hd] fp64, pos [B] (may be negative): HF rotate_half form with fp32 inv_freq (tests/test_gpu_longctx.py _rope64)."""
    hd = x.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = (pos[:, None].float() * inv[None, :]).double()
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1)[:, None], torch.cat([ang.sin(), ang.sin()], -1)[:, None]
    x1, x2 = x[..., : hd // 2], x[..., hd // 2:]
    return x * cos + torch.cat([-x2, x1], -1) * sin


def fused_projection(slabs, ssq, K, eps, bias):
    """(sum of slabs) * rstd + bias in fp64: slabs fp32 [ks, B, W], ssq fp32 [B, nblk], bias fp32 [W] or None.  Returns
    (projection [B, W], magnitude [B, W] = sum |slab| * rstd + |bias|: what the fp32 evaluation's error scales with)."""
    rstd = 1.0 / torch.sqrt(ssq.double().sum(1) / K + eps)
    x = slabs.double().sum(0) * rstd[:, None]
    mag = slabs.double().abs().sum(0) * rstd[:, None]
    if bias is not None:
        x = x + bias.double()[None, :]
        mag = mag + bias.double().abs()[None, :]
    return x, mag


def _neighbours(r: torch.Tensor):
    """The representable values of r's 16-bit type just above and just below each element of r (finite, far from overflow)."""
    bits = r.view(torch.int16).to(torch.int32) & 0xFFFF
    mag, sign = bits & 0x7FFF, bits & 0x8000
    away = ((mag + 1) | sign).to(torch.int16).view(r.dtype).double()                 # one step away from zero
    toward = ((mag - 1).clamp_min(0) | sign).to(torch.int16).view(r.dtype).double()  # one step toward zero
    tiny = torch.tensor([1], dtype=torch.int16).view(r.dtype).double()
    rd = r.double()
    zero = mag == 0
    neg = sign != 0
    up = torch.where(zero, tiny, torch.where(neg, toward, away))
    dn = torch.where(zero, -tiny, torch.where(neg, away, toward))
    up = torch.where((mag == 1) & neg, torch.zeros_like(rd), up)
    dn = torch.where((mag == 1) & ~neg, torch.zeros_like(rd), dn)
    return up, dn


def ambiguous(x: torch.Tensor, mag: torch.Tensor, dtype) -> torch.Tensor:
    """Elements of the fp64 projection x that lie within 2^-20 mag of a rounding boundary of `dtype`: the kernel forms the value
    with at most eight fp32 adds, one multiply, one add and an rsqrt good to 1 ulp - all inside 16 x 2^-24 of mag -, so off this
    set its rounding must equal the fp64 one bit for bit, and on it it may land one step to either side."""
    r = x.to(dtype)
    up, dn = _neighbours(r)
    rd = r.double()
    dist = torch.minimum((x - (rd + up) / 2).abs(), (x - (rd + dn) / 2).abs())
    return dist <= 2.0 ** -20 * mag


def rounds_from_nearby(v: torch.Tensor, x: torch.Tensor, mag: torch.Tensor) -> torch.Tensor:
    """Is the 16-bit value v the rounding of SOME value within 2^-20 mag of x (elementwise)?  v's rounding cell reaches from the
    midpoint with its lower neighbour to the midpoint with its upper one; it must meet [x - tol, x + tol].  Off the ambiguous set
    that leaves the fp64 rounding alone, on it two adjacent values wherever tol is below half a step - and more than two only
    where the sum cancelled to a value so small that the fp32 error spans several steps of the 16-bit type (|x| ~ 1e-4 from
    terms of order 1).  Everything here is exact in fp64."""
    tol = 2.0 ** -20 * mag
    up, dn = _neighbours(v)
    vd = v.double()
    return ((vd + dn) / 2 <= x + tol) & ((vd + up) / 2 >= x - tol)


def one_ulp_apart(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a, b of one 16-bit type: equal or adjacent representable values (elementwise)."""
    up, dn = _neighbours(b)
    ad = a.double()
    return (ad == b.double()) | (ad == up) | (ad == dn)


def reference(c: Ctx, proj, k_hist, v_hist, kstart, L: int, dtype, v_new=None):
    """fp64 decode attention of one launch.  proj [B, width]: the new token's q | k | v projections (any float type; rounded to
    `dtype` first, as the GEMM stores them or as the kernel rounds the fused form); k_hist / v_hist `dtype` [B, nkv, L, hd]
    (slots below kstart[b] may hold anything); kstart int [B].  Position of the new token: L - kstart[b]; keys kstart[b] .. L.
    v_new (optional) `dtype` [B, nkv, hd]: the appended value to use instead of the rounded projection (fused form: where fp32
    cannot decide the rounding, the value the launch itself appended - checked on its own with `rounds_from_nearby`).
    Returns (O [B, nh hd] fp64, k_new fp64 [B, nkv, hd] before its rounding, v_new `dtype` [B, nkv, hd], P [B, nh, L + 1])."""
    B = proj.shape[0]
    nh, nkv, hd, G = c.nh, c.nkv, c.hd, c.G
    p = proj.to(dtype).double()
    kstart = torch.as_tensor(kstart, dtype=torch.long)
    pos = L - kstart
    q = rope64(p[:, : nh * hd].view(B, nh, hd), pos).to(dtype).double()
    kn = rope64(p[:, nh * hd: (nh + nkv) * hd].view(B, nkv, hd), pos)
    v_new = proj.to(dtype)[:, (nh + nkv) * hd:].view(B, nkv, hd) if v_new is None else v_new
    j = torch.arange(L + 1)
    hidden = j[None, :] < kstart[:, None]                                             # [B, L + 1]
    K = torch.cat([k_hist.double(), kn.to(dtype).double()[:, :, None, :]], 2)
    V = torch.cat([v_hist.double(), v_new.double()[:, :, None, :]], 2)
    K = torch.where(hidden[:, None, :, None], torch.zeros_like(K), K)                 # (whatever a hidden slot holds, NaN included)
    V = torch.where(hidden[:, None, :, None], torch.zeros_like(V), V)
    s = torch.einsum("bkgd,bkjd->bkgj", q.view(B, nkv, G, hd), K) * hd ** -0.5
    s = s.masked_fill(hidden[:, None, None, :], -math.inf)
    P = torch.softmax(s, -1)
    O = torch.einsum("bkgj,bkjd->bkgd", P, V).reshape(B, nh * hd)
    return O, kn, v_new, P.reshape(B, nh, L + 1)


# ------------------------------------------------------------------------------------------------ inputs
def nan_like(shape, dtype):
    return torch.full(shape, NAN_BITS, dtype=torch.int16).view(dtype)


def pi_targets(case: Case, b: int):
    """(kind, slot) pairs the peaked family aims queries of row b at: the first visible key, the last cached key, the new key,
    both sides of every 32-slot boundary inside the visible range and the first visible key of every wave's share."""
    L, k0 = case.L, case.kstart_of(b)
    t = [("kstart", k0), ("new", L)]
    if L - 1 >= k0:
        t.append(("last_cached", L - 1))
    for m in range(TILE, L + 1, TILE):
        if m - 1 >= k0:
            t += [(f"below_{m}", m - 1), (f"at_{m}", m)]
    t_first = k0 // TILE
    for tile in range(t_first, L // TILE + 1):
        t.append((f"wave_{(tile - t_first) % WAVES}", max(tile * TILE, k0)))
    return t


def target_kinds(case: Case) -> set:
    return {k for b in range(case.B) for k, _ in pi_targets(case, b)}


def _pi(case: Case, gen) -> torch.Tensor:
    """pi [B, nh]: every kind of target is aimed at by some query of the case (greedy over the rows), the rest cycle through
    their row's targets and uniformly drawn visible slots."""
    nh = case.c.nh
    left = target_kinds(case)
    pi = torch.zeros(case.B, nh, dtype=torch.long)
    for b in range(case.B):
        t = pi_targets(case, b)
        k0 = case.kstart_of(b)
        for h in range(nh):
            want = [x for x in t if x[0] in left]
            if want:
                kind, slot = want[0]
                left.discard(kind)
            elif (b + h) % 2:
                slot = t[(b * nh + h) % len(t)][1]
            else:
                slot = k0 + int(torch.randint(0, case.L - k0 + 1, (1,), generator=gen))
            pi[b, h] = slot
    return pi


def make_inputs(case: Case, dtype=torch.float16):
    """Host tensors of a case.  Always: k_hist / v_hist `dtype` [B, nkv, L, hd] with NaN bit patterns in every slot below
    kstart[b], kstart int32 [B].  random / peaked: qkv `dtype` [B, width] (+ pi [B, nh]).  fused: slabs fp32 [ks, B, width],
    ssq fp32 [B, nblk], bias fp32 [width] or None."""
    c = case.c
    B, L, nh, nkv, hd = case.B, case.L, c.nh, c.nkv, c.hd
    gen = torch.Generator().manual_seed(case.seed)
    kstart = torch.tensor(case.kstart, dtype=torch.int32)
    kh = torch.randn(B, nkv, L, hd, generator=gen)
    vh = torch.randn(B, nkv, L, hd, generator=gen)
    inp = dict(kstart=kstart)
    if case.family == "fused":
        inp["slabs"] = torch.randn(case.ks, B, c.width, generator=gen) * case.ks ** -0.5
        inp["ssq"] = 50.0 + 200.0 * torch.rand(B, case.nblk, generator=gen)
        inp["bias"] = 0.5 * torch.randn(c.width, generator=gen) if case.bias else None
    else:
        qkv = torch.randn(B, c.width, generator=gen)
        if case.family == "peaked":
            kh = (kh * (math.sqrt(hd) / kh.norm(dim=-1, keepdim=True))).to(dtype).float()
            kn = qkv[:, nh * hd: (nh + nkv) * hd].view(B, nkv, hd)
            kn = (kn * (math.sqrt(hd) / kn.norm(dim=-1, keepdim=True))).to(dtype).float()       # the unrotated new key
            qkv[:, nh * hd: (nh + nkv) * hd] = kn.reshape(B, -1)
            pi = _pi(case, gen)
            pos = (L - kstart).long()
            # R(-pos) of a cached (rotated) key; the new key is aimed at through its unrotated form
            kv = torch.arange(nh) // c.G
            aim = kh[torch.arange(B)[:, None], kv[None, :], pi.clamp_max(L - 1)].double()                 # [B, nh, hd]
            q = torch.where((pi < L)[:, :, None], rope64(aim, -pos), kn[:, kv].double())
            qkv[:, : nh * hd] = (ALPHA[hd] * q).float().reshape(B, -1)
            inp["pi"] = pi
        inp["qkv"] = qkv.to(dtype)
    kh, vh = kh.to(dtype), vh.to(dtype)
    hidden = torch.arange(L)[None, :] < kstart[:, None].long()                         # [B, L]
    m = hidden[:, None, :, None].expand(B, nkv, L, hd)
    nan = nan_like((B, nkv, L, hd), dtype)
    inp["k_hist"] = torch.where(m, nan, kh)
    inp["v_hist"] = torch.where(m, nan, vh)
    return inp


def poison_inputs(c: Ctx, B: int, dtype):
    """The launch that leaves NaN in slots 0 .. 159 of rows 0 .. B-1: T0 = 96, step = 63, NaN history, NaN projections."""
    L = CTX_CAP - 1
    return dict(qkv=nan_like((B, c.width), dtype), k_hist=nan_like((B, c.nkv, L, c.hd), dtype), v_hist=nan_like((B, c.nkv, L, c.hd), dtype),
                kstart=torch.zeros(B, dtype=torch.int32), T0=MAX_PROMPT, step=MAX_NEW - 1)


def reference_case(case: Case, inp, dtype, v_new=None):
    """(O, k_new fp64, v_new dtype, P, ambiguous [B, width] bool or None) of a case's inputs."""
    amb = None
    if case.family == "fused":
        x, mag = fused_projection(inp["slabs"], inp["ssq"], case.K, EPS, inp["bias"])
        amb = ambiguous(x, mag, dtype)
        proj = x
    else:
        proj = inp["qkv"]
    return reference(case.c, proj, inp["k_hist"], inp["v_hist"], inp["kstart"], case.L, dtype, v_new) + (amb,)


def peaked_mass(case: Case, inp, P) -> float:
    pi = inp["pi"]
    return float(P.gather(2, pi[:, :, None]).min())


# ------------------------------------------------------------------------------------------------ geometry
def ne_of(hd: int, gp: int) -> int:
    """Rotary pairs a thread stages: the (gp query heads + 1 key) x hd / 2 pairs over 256 threads."""
    return ((gp + 1) * (hd // 2) + 255) // 256


INSTANCE_CELLS = [f"inst.hd{hd}.gp{gp}" for hd in (16, 32, 64, 128) for gp in (1, 2, 4, 8)]
TILING_CELLS = ["ne.1", "ne.2", "ne.3", "idle_waves.0", "idle_waves.1", "idle_waves.2", "idle_waves.3", "tiles_per_wave.1", "tiles_per_wave.2",
                "new_key.index_0", "new_key.index_31", "new_key.index_other", "new_key.alone_in_tile", "new_key.tile_lo>0",
                "t_first==t_new", "first_tile_rerequested", "t_first==t_new.rerequested.lo>0", "new_key.last_slot",
                "group_3.per_head", "group_3.past_threshold"]
FUSED_CELLS = ["form.unfused", "form.fused"] + [f"ks.{k}" for k in range(1, 9)] + ["bias.on", "bias.off", "nblk.<=64", "nblk.<=256", "nblk.>256",
                                                                                  "out_tiled.0", "out_tiled.1"]
REQUIRED = INSTANCE_CELLS + TILING_CELLS + FUSED_CELLS


def geometry_cells(case: Case) -> set:
    """The situations of REQUIRED that the launch of `case` meets, from the kernel's tiling restated: tile t = slots 32 t ..
    32 t + 31; a row's first tile is t_first = kstart / 32, the new key's t_new = L / 32 at index L % 32; wave w takes the tiles
    t_first + w, + 4, ... <= t_new (none: it publishes m = -inf), each as tile(lo, hi) with lo = max(kstart - 32 t, 0); the tile a
    wave requested at entry (t = w) is requested again unless t_first = 0."""
    c = case.c
    cells = {f"inst.hd{c.hd}.gp{case.gp}", f"ne.{ne_of(c.hd, case.gp)}"}
    if c.G == 3:
        cells.add("group_3.past_threshold" if case.B * c.nkv >= GROUP_MIN else "group_3.per_head")
    L = case.L
    t_new, idx = L // TILE, L % TILE
    cells.add("new_key.index_0" if idx == 0 else "new_key.index_31" if idx == 31 else "new_key.index_other")
    if idx == 0:
        cells.add("new_key.alone_in_tile")                  # (kstart < L always: the tile's cached part is empty)
    if L == CTX_CAP - 1:
        cells.add("new_key.last_slot")
    for b in range(case.B):
        k0 = case.kstart_of(b)
        t_first = k0 // TILE
        n = t_new - t_first + 1
        cells.add(f"idle_waves.{max(0, WAVES - n)}")
        cells.add(f"tiles_per_wave.{-(-n // WAVES)}")
        lo = k0 - TILE * t_new
        if lo > 0:
            cells.add("new_key.tile_lo>0")
        if t_first == t_new:
            cells.add("t_first==t_new")
        if t_first > 0:
            cells.add("first_tile_rerequested")
        if t_first == t_new and t_first > 0 and lo > 0:
            cells.add("t_first==t_new.rerequested.lo>0")
    if case.family == "fused":
        cells |= {"form.fused", f"ks.{case.ks}", "bias.on" if case.bias else "bias.off",
                  "nblk.<=64" if case.nblk <= 64 else "nblk.<=256" if case.nblk <= 256 else "nblk.>256", f"out_tiled.{case.out_tiled}"}
    else:
        cells |= {"form.unfused", "out_tiled.0", "out_tiled.1"}
    return cells
