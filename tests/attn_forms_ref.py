"""Reference, inputs and case table of the prefill-attention form tests (tests/test_attn_forms_host.py on the CPU,
tests/test_gpu_attn_forms.py on the GPU).  Plain torch on the CPU; nothing here touches the library.

attn_prefill_kernel is launched in three forms - padded (batch strides, kstart / kend), token-packed (AttnParams::cu) and
token-packed with q_trim - with one or two 16-query tiles per wave (QT), on Q / K / V that are column ranges of one fused
projection buffer.  This module holds
  * `reference`: fp64 softmax-attention of one batch row / protein on the 16-bit operands;
  * two input families per case: `random` (unit-normal Q / K / V) and `peaked` (query i is a multiple of key pi(i), so that
    O[i] = V[pi(i)] up to rounding and a wrong key or V row anywhere is an O(1) error);
  * `geometry_cells`: a restatement of the kernel's tiling that lists which tile / wave / block situations a case reaches;
  * `CASES`: the table, with the QT every case expects from the launcher's rule.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

KB = 64                                   # keys per tile of the kernel
SENTINEL = 0x7B2D                         # 16-bit pattern O is pre-filled with (a finite value in fp16 and in bf16)
GUARD_ROWS = 2                            # rows appended behind the last token of the fused buffer (NaN) and of O (sentinel)
MASS_MIN = 0.99                           # peaked family: reference probability of key pi(i) for every checked query
# peaked family: q = ALPHA k, the score of key pi(i) is ALPHA sqrt(hd) (72 / 45 / 48 / 45).  head_dim 16 needs 18: with 12 the
# smallest mass over this table is 0.974 (two of ~500 random unit vectors in 16 dimensions reach a cosine of 0.9 somewhere among
# the table's ~10^5 queries), with 16 it is 0.9918, with 18 0.9955 in fp16 and in bf16; the largest |q| is then 62, far inside both
ALPHA = {16: 18.0, 32: 8.0, 64: 6.0, 128: 4.0}
LENS = (2, 3, 17, 18, 19, 34, 49, 64, 65, 66, 67, 81, 97, 128, 129, 130, 131, 161, 193, 258, 514)    # the packed batch


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def qt_rule(B: int, heads: int, T: int, hd: int) -> int:
    """The launcher's choice of query tiles per wave (attn_prefill_query_tiles in csrc/attn_prefill.hip), knob misc3 = 0."""
    return 2 if hd <= 64 and B * heads * cdiv(T, 128) >= 512 else 1


@dataclass(frozen=True)
class Case:
    name: str
    form: str                             # "packed" | "padded" | "decoder"
    B: int
    T: int                                # tokens per row (the longest row when packed)
    heads: int
    group: int
    hd: int
    qt: int                               # query tiles per wave the case must run with
    trim: int = 0
    lens: Optional[Tuple[int, ...]] = None      # packed: tokens per protein; padded: kend
    kstart: Optional[Tuple[int, ...]] = None    # decoder
    seed: int = 0

    @property
    def causal(self) -> int:
        return 1 if self.form == "decoder" else 0

    @property
    def knob(self) -> int:
        """Value of knob misc3 that makes the launcher take `qt` at this shape."""
        return 0 if qt_rule(self.B, self.heads, self.T, self.hd) == self.qt else 1

    @property
    def kvh(self) -> int:
        return self.heads // self.group

    @property
    def width(self) -> int:
        """Columns of the fused projection buffer: [q | k | v]."""
        return (self.heads + 2 * self.kvh) * self.hd

    @property
    def cols(self) -> Tuple[int, int, int]:
        return 0, self.heads * self.hd, (self.heads + self.kvh) * self.hd

    @property
    def scale(self) -> float:
        """The encoder pre-scales q by hd^-0.5 and launches with scale 1; the decoder launches with hd^-0.5."""
        return self.hd ** -0.5 if self.form == "decoder" else 1.0

    def row_len(self, b: int) -> int:
        return self.lens[b] if self.form == "packed" else self.T

    def row_start(self, b: int) -> int:
        return sum(self.lens[:b]) if self.form == "packed" else b * self.T

    @property
    def rows(self) -> int:
        return sum(self.lens) if self.form == "packed" else self.B * self.T

    def key_range(self, b: int) -> Tuple[int, int]:
        if self.form == "packed":
            return 0, self.lens[b]
        if self.form == "padded":
            return 0, self.lens[b]
        return self.kstart[b], self.T

    def query_range(self, b: int) -> Tuple[int, int]:
        """Rows of batch row b that the launch computes."""
        n = self.row_len(b)
        return (1, n - 1) if self.trim else (0, n)


def _cases():
    out = []
    seed = 100
    # token-packed, non-causal: the encoder's layout.  21 proteins x 4 heads x 5 blocks of 128 = 420 < 512: QT 1; 5 heads: QT 2
    for hd in (16, 32, 64):
        for qt, heads in ((1, 4), (2, 5)):
            for trim in (0, 1):
                seed += 1
                out.append(Case(f"packed_hd{hd}_qt{qt}_trim{trim}", "packed", len(LENS), max(LENS), heads, 1, hd, qt, trim, lens=LENS,
                                seed=seed))
    # padded, non-causal: the same buffer with batch strides and kend = lens.  15 (batch, head) pairs: not a multiple of 8
    for hd in (16, 64):
        for qt in (1, 2):
            for T, lens in ((130, (130, 129, 65, 17, 1)), (514, (514, 480, 200, 100, 1))):
                seed += 1
                out.append(Case(f"padded_hd{hd}_qt{qt}_T{T}", "padded", 5, T, 3, 1, hd, qt, lens=lens, seed=seed))
    # decoder prefill: causal, left-padded (kstart), GQA, [B T, (nh + 2 nkv) hd]
    ks8 = (0, 1, 63, 64, 65, 100, 129, 128)
    dec = [("dec_hd128_qt1", 3, 257, 8, 4, 128, 1, (0, 64, 256)),
           ("dec_hd64_qt2", 8, 130, 32, 4, 64, 2, ks8),
           ("dec_hd16_qt2", 8, 130, 32, 2, 16, 2, ks8[3:] + ks8[:3]),
           ("dec_hd32_qt1", 2, 130, 4, 1, 32, 1, (1, 65)),
           ("dec_hd32_qt2", 2, 130, 4, 1, 32, 2, (63, 100))]
    for name, B, T, heads, group, hd, qt, ks in dec:
        seed += 1
        out.append(Case(name, "decoder", B, T, heads, group, hd, qt, kstart=ks, seed=seed))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------ reference
def attention_probs(q, k, *, scale, group, causal=False, kstart=0, kend=None):
    """Softmax probabilities [heads, T, T] in fp64 of one batch row: q [T, heads, hd], k [T, heads / group, hd] (any dtype; used
    as fp64).  Key j is visible to query i iff kstart <= j < kend and (not causal or j <= i); a query without a visible key has
    an all-zero row."""
    T, heads, hd = q.shape
    kend = T if kend is None else kend
    q, k = q.double(), k.double()
    j = torch.arange(T)
    vis = ((j >= kstart) & (j < kend))[None, :].repeat(T, 1)
    if causal:
        vis &= j[None, :] <= j[:, None]
    P = torch.zeros(heads, T, T, dtype=torch.float64)
    for h in range(heads):
        s = (q[:, h] @ k[:, h // group].T) * scale
        s = torch.where(vis, s, torch.full_like(s, -math.inf))
        m = s.max(dim=1, keepdim=True).values
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        e = torch.exp(s - m)                                          # (masked keys: exp(-inf) = 0)
        den = e.sum(dim=1, keepdim=True)
        P[h] = torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))
    return P


def reference(q, k, v, *, scale, group, causal=False, kstart=0, kend=None, trim=0):
    """fp64 attention of one batch row.  Returns (out [T, heads, hd] fp64, computed [T] bool, has_key [T] bool, P):
    computed = rows the launch writes (all but the first and the last with trim), has_key = rows with a visible key."""
    T, heads, hd = q.shape
    P = attention_probs(q, k, scale=scale, group=group, causal=causal, kstart=kstart, kend=kend)
    vv = v.double()
    out = torch.stack([P[h] @ vv[:, h // group] for h in range(heads)], dim=1)
    has_key = P[0].sum(dim=1) > 0
    computed = torch.ones(T, dtype=torch.bool)
    if trim:
        computed[0] = False
        computed[T - 1] = False
    return out, computed, has_key, P


# ------------------------------------------------------------------------------------------------ inputs
def pi_targets(case: Case, b: int):
    """Keys of row b that the peaked family must aim some checked query at: the first visible key, the row's last key and both
    sides of every 64-key tile boundary inside the visible range."""
    k0, k1 = case.key_range(b)
    t = {k0, k1 - 1}
    for m in range(KB, k1, KB):
        if m - 1 >= k0:
            t |= {m - 1, m}
    return sorted(t)


def _pi_row(case: Case, b: int, gen) -> torch.Tensor:
    """pi [heads, T] for row b: the key query (i, h) is aimed at; -1 for a query without a visible key."""
    n = case.row_len(b)
    k0, k1 = case.key_range(b)
    pi = torch.full((case.heads, n), -1, dtype=torch.long)
    targets = pi_targets(case, b)
    if not case.causal:
        q0, q1 = case.query_range(b)
        for h in range(case.heads):
            perm = torch.randperm(k1, generator=gen)
            if case.trim and n >= 16:
                # the unchecked first / last query must not be the only ones aimed at a target: trade places with an interior one
                for edge in (0, n - 1):
                    if int(perm[edge]) in targets:
                        for i in range(q0, q1):
                            if int(perm[i]) not in targets:
                                perm[[edge, i]] = perm[[i, edge]]
                                break
            pi[h] = perm[torch.arange(n) % k1]                        # (padded rows: queries past kend wrap around)
        return pi
    bounds = [t for t in targets if t % KB in (0, KB - 1) and t not in (k0, k1 - 1)] or [k0]
    for h in range(case.heads):
        for i in range(k0, n):
            mode = (i + h) % 4
            if mode == 0:
                pi[h, i] = i                                           # the diagonal: the last key the query may see
            elif mode == 1:
                pi[h, i] = k0                                          # the first visible key
            elif mode == 2:
                ok = [t for t in bounds if t <= i]
                pi[h, i] = ok[(i // 4 + h) % len(ok)] if ok else i
            else:
                pi[h, i] = k0 + int(torch.randint(0, i - k0 + 1, (1,), generator=gen))
    return pi


def make_inputs(case: Case, family: str, dtype=torch.float16):
    """Host tensors of a case: `qkv` [rows + GUARD_ROWS, width] in `dtype` (the guard rows NaN: nothing may read them), the
    per-row views q / k / v in `dtype`, `pi` per row (peaked) and the int32 arrays the launch needs."""
    assert family in ("random", "peaked")
    gen = torch.Generator().manual_seed(case.seed * 2 + (family == "peaked"))
    hd, heads, kvh = case.hd, case.heads, case.kvh
    qkv = torch.full((case.rows + GUARD_ROWS, case.width), float("nan"), dtype=dtype)
    cq, ck, cv = case.cols
    rows, pis = [], []
    for b in range(case.B):
        n = case.row_len(b)
        q = torch.randn(n, heads, hd, generator=gen)
        k = torch.randn(n, kvh, hd, generator=gen)
        v = torch.randn(n, kvh, hd, generator=gen)
        pi = None
        if family == "peaked":
            k = (k * (math.sqrt(hd) / k.norm(dim=-1, keepdim=True))).to(dtype)
            pi = _pi_row(case, b, gen)
            pre = hd ** -0.5 if case.form != "decoder" else 1.0
            for h in range(heads):
                aimed = pi[h] >= 0
                q[aimed, h] = ALPHA[hd] * pre * k[pi[h][aimed], h // case.group].float()
        q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
        r0 = case.row_start(b)
        qkv[r0:r0 + n, cq:cq + heads * hd] = q.reshape(n, -1)
        qkv[r0:r0 + n, ck:ck + kvh * hd] = k.reshape(n, -1)
        qkv[r0:r0 + n, cv:cv + kvh * hd] = v.reshape(n, -1)
        rows.append((q, k, v))
        pis.append(pi)
    cu = None
    if case.form == "packed":
        cu = torch.tensor([case.row_start(b) for b in range(case.B)] + [case.rows], dtype=torch.int32)
    kend = torch.tensor(case.lens, dtype=torch.int32) if case.form == "padded" else None
    kstart = torch.tensor(case.kstart, dtype=torch.int32) if case.form == "decoder" else None
    return dict(qkv=qkv, rows=rows, pi=pis, cu=cu, kstart=kstart, kend=kend)


def reference_case(case: Case, inp, trim: Optional[int] = None):
    """Per batch row: (out, computed, has_key, P) of `reference` on the row's 16-bit operands."""
    trim = case.trim if trim is None else trim
    res = []
    for b, (q, k, v) in enumerate(inp["rows"]):
        k0, k1 = case.key_range(b)
        res.append(reference(q, k, v, scale=case.scale, group=case.group, causal=bool(case.causal), kstart=k0, kend=k1, trim=trim))
    return res


def peaked_mass(case: Case, inp, ref) -> float:
    """Smallest reference probability of key pi(i) over every query the launch computes that has a visible key."""
    worst = 1.0
    for b in range(case.B):
        out, computed, has_key, P = ref[b]
        pi = inp["pi"][b]
        chk = computed & has_key
        for h in range(case.heads):
            idx = chk.nonzero()[:, 0]
            assert bool((pi[h][idx] >= 0).all())
            worst = min(worst, float(P[h][idx, pi[h][idx]].min()) if len(idx) else 1.0)
    return worst


def pi_misses(case: Case, inp):
    """(row, key) pairs of pi_targets that no checked query of the row is aimed at, over the rows with at least 16 checked
    queries (a protein of 3 tokens has one query: it cannot reach two keys)."""
    miss = []
    for b in range(case.B):
        q0, q1 = case.query_range(b)
        k0, _ = case.key_range(b)
        q0 = max(q0, k0) if case.causal else q0
        if q1 - q0 < 16:
            continue
        hit = set(inp["pi"][b][:, q0:q1].reshape(-1).tolist())
        miss += [(b, t) for t in pi_targets(case, b) if t not in hit]
    return miss


# ------------------------------------------------------------------------------------------------ geometry
KEY_CELLS = ["keys.tiles.1", "keys.tiles.2", "keys.tiles.3+", "keys.last.1-16", "keys.last.17-32", "keys.last.33-63", "keys.last.64",
             "keys.none_for_block"]
KSTART_CELLS = ["kstart.0", "kstart.inside_first_tile", "kstart.on_tile_boundary", "kstart.T-1"]
QUERY_CELLS = ["last_block.waves.1", "last_block.waves.2", "last_block.waves.3", "last_block.waves.4", "wave.first_tile_clamped",
               "packed.block_past_row_end", "grid.bh_not_multiple_of_8", "trim.row_of_2.no_query", "trim.row_of_3.one_query",
               "trim.saves_a_block", "trim.last_block_of_one_query"]
ALL_CELLS = KEY_CELLS + KSTART_CELLS + [f"qt{qt}.{c}" for qt in (1, 2) for c in QUERY_CELLS] + ["qt2.wave.second_tile_dead"]


def geometry_cells(case: Case) -> set:
    """The situations of ALL_CELLS that the launch of `case` meets, from the kernel's tiling restated: a workgroup is 4 waves of
    QW = 16 QT queries, QB = 64 QT queries of one (batch row, head); the grid has cdiv(T - 2 trim, QB) blocks per (row, head) for
    ceil(B heads / 8) 8 pairs; block `blk` of row b starts at query blk QB + trim and walks the key tiles of 64 from
    kstart / 64 * 64 to kend (causal: to the block's last query), a last tile of <= 16 / <= 32 keys as 1 / 2 sixteen-key
    subtiles, anything longer as a whole tile."""
    QT = case.qt
    QW, QB = 16 * QT, 64 * QT
    pre = f"qt{QT}."
    cells = set()
    if (case.B * case.heads) % 8:
        cells.add(pre + "grid.bh_not_multiple_of_8")
    trim = case.trim
    nqb = cdiv(case.T - 2 * trim, QB)
    for b in range(case.B):
        n = case.row_len(b)
        Tq = n - trim if case.form == "packed" else n
        k0, k1 = case.key_range(b)
        if case.form == "decoder":
            if k0 == 0:
                cells.add("kstart.0")
            elif k0 == n - 1:
                cells.add("kstart.T-1")
            elif k0 % KB == 0:
                cells.add("kstart.on_tile_boundary")
            elif k0 < KB:
                cells.add("kstart.inside_first_tile")
        if trim:
            if n == 2:
                cells.add(pre + "trim.row_of_2.no_query")
            if n == 3:
                cells.add(pre + "trim.row_of_3.one_query")
            if cdiv(n - 2, QB) < cdiv(n, QB):
                cells.add(pre + "trim.saves_a_block")
            if n > 3 and (n - 2) % QB == 1:
                cells.add(pre + "trim.last_block_of_one_query")
        for blk in range(nqb):
            q0 = blk * QB + trim
            if q0 >= Tq:
                assert case.form == "packed"
                cells.add(pre + "packed.block_past_row_end")
                continue
            live = [w for w in range(4) if q0 + w * QW < Tq]
            if q0 + QB >= Tq:
                cells.add(pre + f"last_block.waves.{len(live)}")
            for w in live:
                qw = q0 + w * QW
                if qw + 16 > Tq:
                    cells.add(pre + "wave.first_tile_clamped")
                if QT == 2 and qw + 16 >= Tq:
                    cells.add("qt2.wave.second_tile_dead")
            k_lo, k_hi = k0 // KB * KB, k1
            if case.causal:
                k_hi = min(k_hi, min(q0 + QB - 1, n - 1) + 1)
            if k_lo >= k_hi:
                cells.add("keys.none_for_block")
                continue
            nt = cdiv(k_hi - k_lo, KB)
            last = k_hi - k_lo - KB * (nt - 1)
            cells.add("keys.tiles." + ("1" if nt == 1 else "2" if nt == 2 else "3+"))
            cells.add("keys.last." + ("1-16" if last <= 16 else "17-32" if last <= 32 else "33-63" if last < KB else "64"))
    return cells
