"""Sampling head (row N1).  TEST INFRASTRUCTURE.

The reference samples by default (eval/run_opus_ddp.py:126-128,156-157: do_sample when temperature > 0,
temperature 0.1, top_p 0.7) through transformers' GenerationMixin: TemperatureLogitsWarper, TopPLogitsWarper,
softmax, torch.multinomial (local copy: transformers/generation/logits_process.py:515-540).  This restates the
distribution the next token is drawn from; the draw itself depends on the RNG, so parity is distributional.
"""
import numpy as np
import torch


def _warp(scores: torch.Tensor, top_p: float, top_k: int, min_keep: int = 1) -> torch.Tensor:
    """TopKLogitsWarper then TopPLogitsWarper on already temperature-scaled scores [B,V]: filtered entries -> -inf.
    min_keep = the warpers' min_tokens_to_keep: 1 when sampling one sequence; with num_beams > 1 GenerationMixin builds both with
    #eos + 1 (2 without an EOS id) - generation/utils.py _get_logits_processor, "keep at least one non-eos token"."""
    if top_k and top_k > 0:                                       # logits_process.py TopKLogitsWarper: ties with the k-th stay
        k = min(max(int(top_k), int(min_keep)), scores.shape[-1])
        scores = scores.masked_fill(scores < torch.topk(scores, k)[0][..., -1, None], float("-inf"))
    sorted_logits, sorted_idx = torch.sort(scores, descending=False)
    cum = sorted_logits.softmax(-1).cumsum(-1)
    remove = cum <= (1 - top_p)
    remove[..., -int(min_keep):] = False                       # min_tokens_to_keep
    mask = remove.scatter(1, sorted_idx, remove)
    return scores.masked_fill(mask, float("-inf"))


def beam_sample_distribution(logits: torch.Tensor, run_scores: torch.Tensor, temperature: float, top_p: float,
                             top_k: int = 0, min_keep: int = 2) -> torch.Tensor:
    """Beam-sample (GenerationMixin._beam_search with do_sample; generation/utils.py: log_softmax, the warpers on the
    log-probabilities, + running beam scores, softmax over the flattened [K V]): fp32 logits [K,V] of one batch row's beams and
    their running scores [K] -> the probabilities [K V] the FIRST of the M continuations is drawn from (torch.multinomial
    without replacement draws the next ones from the same weights with the drawn entries removed).  min_keep = #eos + 1, at
    least 2: the min_tokens_to_keep GenerationMixin gives both warpers under beam-sample."""
    lp = torch.log_softmax(logits.float(), dim=-1) / temperature
    lp = _warp(lp, top_p, top_k, min_keep)
    return (lp + run_scores.float()[:, None]).reshape(-1).softmax(-1)


def sampling_distribution(logits: torch.Tensor, temperature: float, top_p: float, top_k: int = 0) -> torch.Tensor:
    """fp32 logits [B,V] -> probabilities [B,V] after temperature, top-k (0 = off: transformers >= 5's default; 4.46.3, the
    reference's pin, defaults to 50) and nucleus filtering."""
    scores = logits / temperature
    if top_k and top_k > 0:
        return _warp(scores, top_p, top_k).softmax(-1)
    sorted_logits, sorted_idx = torch.sort(scores, descending=False)
    cum = sorted_logits.softmax(-1).cumsum(-1)
    remove = cum <= (1 - top_p)
    remove[..., -1:] = False                                   # min_tokens_to_keep = 1
    mask = remove.scatter(1, sorted_idx, remove)
    return scores.masked_fill(mask, float("-inf")).softmax(-1)


# ------------------------------------------------------------------------------------------------ draw-level reference
# The device head draws from a counter-based generator, so every draw is a pure function of (seed, row, step) and the host can
# name the token it must pick.  What follows restates that rule in fp64, with a per-token margin that says when the fp32
# kernel's answer may legitimately differ (a "non-decisive" draw).
M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_BEAM_STRIDE = 0xD1B54A32D192ED03
_MUL1, _MUL2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_MUL1_INV, _MUL2_INV = pow(_MUL1, -1, 1 << 64), pow(_MUL2, -1, 1 << 64)
U24 = 1 << 24
EPS32 = 2.0 ** -24                      # unit roundoff of fp32


def splitmix64(x: int) -> int:
    x = (x + _GOLDEN) & M64
    x = ((x ^ (x >> 30)) * _MUL1) & M64
    x = ((x ^ (x >> 27)) * _MUL2) & M64
    return x ^ (x >> 31)


def _unxorshift(y: int, s: int) -> int:
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def splitmix64_inv(y: int) -> int:
    x = _unxorshift(y & M64, 31)
    x = (x * _MUL2_INV) & M64
    x = _unxorshift(x, 27)
    x = (x * _MUL1_INV) & M64
    x = _unxorshift(x, 30)
    return (x - _GOLDEN) & M64


def _row_key(row: int, step: int) -> int:
    return ((_GOLDEN * (row + 1)) & M64) ^ (((step + 1) << 32) & M64)


def draw_uniform(seed: int, row: int, step: int):
    """(k, u) of sample_stage2_kernel's draw for (seed, row, step): the 24-bit index k = h >> 40 and u = k / 2^24."""
    k = splitmix64((seed ^ _row_key(row, step)) & M64) >> 40
    return k, k / U24


def seed_for_uniform(k: int, row: int, step: int, low: int = 0x3C6EF372FE) -> int:
    """A seed whose draw for (row, step) has the 24-bit index k (splitmix64 is a bijection: invert it on a chosen hash)."""
    h = ((int(k) & (U24 - 1)) << 40) | (low & ((1 << 40) - 1))
    return splitmix64_inv(h) ^ _row_key(row, step)


def beam_uniforms(seed: int, step: int, row: int, V: int) -> np.ndarray:
    """beam_sample_kernel's per-token uniforms of decoder row `row`, bit for bit (fp32: ((h >> 41) + 0.5f) / 2^23, in (0, 1))."""
    h0 = np.uint64(splitmix64((seed ^ _row_key(row, step)) & M64))
    with np.errstate(over="ignore"):
        x = h0 + np.uint64(_BEAM_STRIDE) * (np.arange(V, dtype=np.uint64) + np.uint64(1))
        x = x + np.uint64(_GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(_MUL1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(_MUL2)
        x = x ^ (x >> np.uint64(31))
    k = (x >> np.uint64(41)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(2.0 ** -23)


# Margins (relative, per token; stated once here and used by every draw-level test):
#   exponent: the kernel forms x = l * (1/T) - max * (1/T) in fp32 (1/T rounded, each product and the difference rounded) and takes
#     __expf(x) = exp2(x * log2 e) (one more rounding, then ~1 ulp): |dp / p| <= 2^-23 (|l| + |max|) / T + 2^-22 |x| + 2^-21,
#     and 0 when x is exactly 0 (l == max: p = 1 exactly);
#   sums: an fp32 sum of positive terms over a chain of n additions is off by at most 4 sqrt(n) + 8 units of 2^-24 relative (the
#     worst case is n units; round-to-nearest errors of a chain add like a random walk, and this is > 10 of its standard
#     deviations), and exactly 0 when every term is a multiple of 2^e and the sum stays below 2^(e + 24);
#   the bisection branch (more than EXACT_CAP candidates) resolves a threshold to 2^-40 on p: an absolute slack on comparisons;
#   top-k with no more candidates than k: the kernel leaves the non-candidate members of the top-k set out of Z (each of them has
#     p <= (1 - top_p) / V): their summed mass widens the nucleus cut.
EXACT_CAP, LDS_CAP, APART = 1024, 6144, 64


def _sum_margin(n: int) -> float:
    return (4.0 * np.sqrt(max(n, 1)) + 8.0) * EPS32


def _exact_sum(p: np.ndarray) -> bool:
    """Every fp32 partial sum of these terms is exact (whatever the order)."""
    p = p[p > 0]
    if p.size == 0:
        return True
    m, e = np.frexp(p)                                      # p = m 2^e, 0.5 <= m < 1
    scaled = np.ldexp(m, 24)                                 # integer iff p has <= 24 significant bits
    if not np.all(scaled == np.floor(scaled)):
        return False
    tz = np.array([(int(s) & -int(s)).bit_length() - 1 for s in scaled.astype(np.int64)])
    lsb = int((e - 24 + tz).min())                           # every term is a multiple of 2^lsb
    return float(p.sum()) < 2.0 ** (lsb + 24)


class HeadRef:
    """fp64 restatement of the sampling head for ONE row of fp32 logits: HF's TemperatureLogitsWarper, TopKLogitsWarper (ties with the
    k-th stay; k = max(top_k, min_keep)) and TopPLogitsWarper (ascending cumulative mass, at least min_keep top tokens kept), then CDF
    inversion in index order: the first kept i whose cumulative kept mass exceeds u * total.

    A kept / dropped decision is certain when it holds for every perturbation of the p_i within the margins above; `kept` are the
    tokens kept for certain, `maybe` the tokens kept under some admissible perturbation (kept included).  `tie_cut`: the nucleus cut
    falls inside a tie (HF's sort order decides there; the kernel keeps or drops the whole tie): no draw of the row is decisive."""

    def __init__(self, logits, temperature: float, top_p: float, top_k: int = 0, min_keep: int = 1):
        l = np.asarray(logits, dtype=np.float32).astype(np.float64)
        V = l.size
        T = float(np.float32(temperature))
        tp = float(np.float32(top_p))
        self.V, self.T, self.top_p = V, T, tp
        lmax = l.max()
        with np.errstate(invalid="ignore"):
            x = np.where(np.isfinite(l), (l - lmax) / T, -np.inf)
        p = np.exp(x)
        xf = np.where(np.isfinite(x), x, 0.0)
        d = 2.0 ** -23 * (np.abs(np.where(np.isfinite(l), l, 0.0)) + abs(lmax)) / T + 2.0 ** -22 * np.abs(xf) + 2.0 ** -21
        d = np.where(x == 0, 0.0, d)
        d = np.where(p < 1e-30, 1.0, d)                         # (fp32 underflow: the kernel may hold 0)
        thr = (1.0 - tp) / V
        self.nc = int((p > thr).sum())
        # tokens that are certainly no candidate (p (1 + d) <= (1 - top_p) / V) are never kept: only their mass counts
        live = p * (1 + d) > thr
        if min_keep > 1:                                          # (the min_keep best tokens stay whatever their p)
            live |= l >= np.sort(l)[-min_keep]
        full_l, full_V, live_idx = l, V, np.nonzero(live)[0]
        dead_lo, dead_hi = float((p * (1 - d)).clip(min=0)[~live].sum()), float((p * (1 + d))[~live].sum())
        l, p, d, x = l[live], p[live], d[live], x[live]
        nL = live_idx.size
        cand_lo = p * (1 - d) > thr                               # a stage-1 candidate for certain / possibly
        cand_hi = p * (1 + d) > thr
        self.nc_range = (int(cand_lo.sum()), int(cand_hi.sum()))
        nc = self.nc
        bis = nc > EXACT_CAP
        slack = 2.0 ** -38 if bis else 0.0
        # chains of additions: stage 1 (a thread's values, 256-way tree, 64 parts), stage 2 (exact rank: nc serial; bisection: nc / 256
        # serial + tree), the draw (a thread's chunk + the scan + the owner's walk)
        tper = -(-(-(-V // APART) + 3) // 4 * 4 // 256)
        n_nuc = max(nc, 1) if not bis else -(-nc // 256) + 8
        n_nuc += tper + 8 + APART
        cper = max(1, -(-nc // 256))
        exact = _exact_sum(p[p > thr].astype(np.float32).astype(np.float64)) and np.all(d[p > thr] == 0)
        g_nuc = 0.0 if exact else _sum_margin(n_nuc)
        self.g_draw = 0.0 if exact else _sum_margin(2 * cper + 12)
        plo, phi = p * (1 - d) - slack, p * (1 + d) + slack       # orderings
        mlo, mhi = np.maximum(p * (1 - d), 0.0), p * (1 + d)      # masses
        # top-k (k = max(top_k, min_keep) when top_k > 0; ties with the k-th stay): count of tokens strictly more probable
        k = max(int(top_k), int(min_keep)) if top_k and top_k > 0 else 0
        if 0 < k < full_V:
            order_lo = np.sort(plo)
            order_hi = np.sort(phi)
            above_def = nL - np.searchsorted(order_lo, phi, side="right")          # p_i^lo > p_j^hi
            above_pos = nL - np.searchsorted(order_hi, plo, side="right")          # p_i^hi > p_j^lo (self and exact ties included)
            _, inv, cnt = np.unique(l, return_inverse=True, return_counts=True)
            above_pos = above_pos - cnt[inv]                                         # exact ties are never above (the same fp32 p)
            in_k, maybe_k = above_pos < k, above_def < k
            # the kernel's top-k works on the candidates; with at most k of them it keeps them all and Z is theirs alone
            dead_k = dead_hi if nL < k else 0.0                     # (fewer live tokens than k: dead ones fill the top-k set)
            missing = float(mhi[maybe_k & ~cand_lo].sum()) + dead_k
            Zlo, Zhi = float(mlo[in_k].sum()) - missing, float(mhi[maybe_k].sum()) + dead_k
            below_lo, below_hi = 0.0, dead_k
        else:
            in_k = maybe_k = np.ones(nL, dtype=bool)
            missing = 0.0
            Zlo, Zhi = float(mlo.sum()) + dead_lo, float(mhi.sum()) + dead_hi
            below_lo, below_hi = dead_lo, dead_hi                 # (the kernel's S0: the non-candidates' mass)
        Zlo, Zhi = Zlo * (1 - g_nuc), Zhi * (1 + g_nuc)
        cut_lo, cut_hi = (1 - tp) * Zlo, (1 - tp) * Zhi
        # nucleus: A_j = mass of the (top-k) tokens with p <= p_j, ties included; keep iff A_j > cut
        idx = np.nonzero(maybe_k)[0]
        o = idx[np.argsort(p[idx], kind="stable")]
        # A_j^-: tokens certainly in top-k and certainly <= p_j (p_i^hi <= p_j^lo, or an exact tie); A_j^+: possibly so
        cert = in_k[o]
        s_lo = np.argsort(phi[o], kind="stable")
        cum_lo = np.concatenate([[0.0], np.cumsum(np.where(cert[s_lo], mlo[o][s_lo], 0.0))])
        s_hi = np.argsort(plo[o], kind="stable")
        cum_hi = np.concatenate([[0.0], np.cumsum(mhi[o][s_hi])])
        lo_sorted, hi_sorted = phi[o][s_lo], plo[o][s_hi]
        pj_lo, pj_hi = plo[o], phi[o]
        A_lo = cum_lo[np.searchsorted(lo_sorted, pj_lo, side="right")]
        A_hi = cum_hi[np.searchsorted(hi_sorted, pj_hi, side="right")]
        # exact ties (same logit) are always <= each other
        lv = l[o]
        _, inv_t, cnt_t = np.unique(lv, return_inverse=True, return_counts=True)
        tm = cnt_t[inv_t] * p[o]                                   # mass of the token's tie group
        A_lo = A_lo + np.where(cert, tm * (1 - d[o]), 0.0) - missing + below_lo   # (ties are never in the first sum)
        A_hi = A_hi + below_hi
        A_lo, A_hi = A_lo * (1 - g_nuc), A_hi * (1 + g_nuc)
        keep_c = cert & (A_lo > cut_hi) & cand_lo[o]
        keep_m = (A_hi > cut_lo) & cand_hi[o]
        if min_keep > 1:                                           # the min_keep best tokens stay whatever the nucleus says
            top = np.argsort(-l, kind="stable")[:min_keep]
            lm = l[top[-1]]
            keep_c |= (l[o] >= lm) & cert
            keep_m |= l[o] >= lm
        self.kept = np.zeros(full_V, dtype=bool)
        self.maybe = np.zeros(full_V, dtype=bool)
        self.kept[live_idx[o[keep_c]]] = True
        self.maybe[live_idx[o[keep_m]]] = True
        self.maybe |= self.kept
        # the nucleus cut inside a tie: p_below + p <= cut < p_below + |G| p for a tie group G (at some admissible perturbation);
        # a tie group is a run of equal logits in the ascending order o
        self.tie_cut = False
        if lv.size:
            start = np.concatenate([[True], lv[1:] != lv[:-1]])
            gid = np.cumsum(start) - 1
            n_g = np.bincount(gid)
            below = np.concatenate([[0.0], np.cumsum(np.where(cert, p[o], 0.0))])[np.nonzero(start)[0]]
            pg = p[o][start]
            below = below + below_lo
            risky = (n_g >= 2) & (below + pg <= cut_hi) & (below + n_g * pg > cut_lo) & self.maybe[live_idx[o[start]]] \
                & np.isfinite(lv[start])
            if min_keep > 1:
                risky &= ~(lv[start] >= lm)
            self.tie_cut = bool(risky.any())
        p_full, d_full = np.zeros(full_V), np.ones(full_V)
        p_full[live_idx], d_full[live_idx] = p, d
        p, d = p_full, d_full
        mlo, mhi = np.maximum(p * (1 - d), 0.0), p * (1 + d)
        self.p, self.d = p, d
        self.undecided = int((self.maybe & ~self.kept).sum())
        # CDF bounds over the possibly-kept tokens in index order
        ids = np.nonzero(self.maybe)[0]
        g = self.g_draw
        self.ids = ids
        self.C_lo = np.cumsum(np.where(self.kept[ids], mlo[ids], 0.0)) * (1 - g)
        self.C_hi = np.cumsum(mhi[ids]) * (1 + g)
        self.C = np.cumsum(np.where(self.kept[ids], p[ids], 0.0))
        self.total_lo, self.total_hi, self.total = self.C_lo[-1], self.C_hi[-1], self.C[-1]

    def draw(self, u):
        """u: array of uniforms (k / 2^24) -> (id the fp64 rule picks, decisive flag, lowest and highest admissible id)."""
        u = np.asarray(u, dtype=np.float64)
        t = u * self.total
        t_lo = u * self.total_lo * (1 - EPS32)                  # (target = u * total: one fp32 rounding)
        t_hi = u * self.total_hi * (1 + EPS32)
        ids = self.ids
        pick = ids[np.minimum(np.searchsorted(self.C, t, side="right"), ids.size - 1)]
        # token j (position q) is admissible iff C_lo[q - 1] <= t_hi and C_hi[q] > t_lo
        q_min = np.searchsorted(self.C_hi, t_lo, side="right")
        C_lo_prev = np.concatenate([[0.0], self.C_lo[:-1]])
        q_max = np.searchsorted(C_lo_prev, t_hi, side="right") - 1
        q_min = np.minimum(q_min, ids.size - 1)
        q_max = np.clip(q_max, 0, ids.size - 1)
        decisive = (q_min == q_max) & self.kept[ids[q_max]] & (ids[q_max] == pick) & (not self.tie_cut)
        return pick, decisive, ids[q_min], ids[q_max]

    def admissible(self, token: int, lo_id: int, hi_id: int) -> bool:
        """`token` is a possibly-kept id between the lowest and the highest admissible id of its draw."""
        return 0 <= token < self.V and bool(self.maybe[token]) and lo_id <= token <= hi_id

    def boundaries(self):
        """Interior CDF boundaries of the kept set as fractions of the total (between consecutive certainly-kept tokens)."""
        return self.C[:-1][self.kept[self.ids][:-1]] / self.total


def beam_reference(logits, run, temperature: float, top_p: float, top_k: int, M: int, seed: int, step: int, b: int,
                   refs=None):
    """Beam-sample's M draws of batch row b from its K decoder rows (fp32 logits [K, V], running scores [K]): the M largest keys
    a(k, v) - log(-log u_kv) over the warpers' kept sets (min_tokens_to_keep = M / K), a = (l - lse) / T + run, ties to the lower
    flat id k V + v.  Returns (flat ids in order, decisive).  Decisive: the top M + 1 keys of the possibly-kept tokens hold certainly
    kept tokens in their first M places and every consecutive gap exceeds the two keys' margins (a: 2^-22 (|l| + |lse|) / T +
    2^-23 (|run| + |a|); the Gumbel term from the exact fp32 u: 2^-21 + 2^-22 / (-log u) relative on -log u, then 2^-21 (1 + |g|))."""
    logits = np.asarray(logits, dtype=np.float32)
    K, V = logits.shape
    T = float(np.float32(temperature))
    keys, margins, flat, cert = [], [], [], []
    for k in range(K):
        ref = refs[k] if refs is not None else HeadRef(logits[k], temperature, top_p, top_k, min_keep=max(1, M // K))
        l = logits[k].astype(np.float64)
        lse = float(np.log(np.exp(l - l.max()).sum()) + l.max())
        ids = np.nonzero(ref.maybe)[0]
        a = (l[ids] - lse) / T + float(run[k])
        uu = beam_uniforms(seed, step, b * K + k, V)[ids].astype(np.float64)
        w = -np.log(uu)
        gmb = -np.log(w)
        dw = (2.0 ** -21 + 2.0 ** -22 / w)
        ma = 2.0 ** -22 * (np.abs(l[ids]) + abs(lse)) / T + 2.0 ** -23 * (abs(float(run[k])) + np.abs(a)) + 2.0 ** -20
        mg = dw + 2.0 ** -21 * (1 + np.abs(gmb))
        keys.append(a + gmb)
        margins.append(ma + mg)
        flat.append(k * V + ids)
        cert.append(ref.kept[ids])
    keys, margins, flat, cert = map(np.concatenate, (keys, margins, flat, cert))
    order = np.lexsort((flat, -keys))[:M + 1]
    top = flat[order[:M]]
    decisive = bool(cert[order[:M]].all())
    for i in range(min(M, order.size - 1)):
        a_, b_ = order[i], order[i + 1]
        if keys[a_] - keys[b_] <= margins[a_] + margins[b_]:
            decisive = False
    return top, decisive
