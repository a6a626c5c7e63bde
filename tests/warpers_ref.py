"""fp64 restatement of the sampling warpers behind top-k / top-p (opus_set_sampling_warpers).  TEST INFRASTRUCTURE.

Layered on oracle.sampling: HeadRef gives p_i = exp(l_i / T - max / T), the per-token relative margin d_i of the kernel's fp32 p, and
the sets top-k / top-p keep for certain (`kept`) and possibly (`maybe`).  WarpRef narrows both sets through transformers' chain
MinP -> Typical -> Epsilon -> Eta (min_tokens_to_keep = 1; every warper sees the softmax over what the earlier ones kept):

    min_p m:      keep p >= m                                 (m times the largest p, which is 1)
    typical t:    Z = sum p, A = sum p log p, c = A / Z, d_i = |c - log p_i| (= |-log q_i - H|);
                  keep i iff the mass of the tokens strictly nearer (d_j < d_i) is below t Z
                  (= the smallest prefix in ascending d that reaches t, the crossing token and its ties included)
    epsilon e:    keep p >= min(e Z, max p)
    eta e':       H = log Z - A / Z; keep p >= min(min(e', sqrt(e') exp(-H)) Z, max p)

Every token ends as surely kept, surely removed or borderline (`maybe` and not `kept`).  A decision is sure when it holds for every
value the kernel's fp32 quantities can take.  Margins, from the unit round-off u = 2^-24 and the number of summed terms:

    p:    HeadRef's d_i (relative).
    log:  logf is correctly rounded to 1 ulp, its argument carries d_i:  |dlog p_i| <= 1.01 d_i + 4 u |log p_i|  (0 at p = 1).
    sums: a chain of n fp32 additions of same-signed terms is off by at most (4 sqrt(n) + 8) u relative - oracle.sampling's bound
          for the head's own sums (the worst case is n u; round-to-nearest errors add like a random walk, and this is > 10 of its
          standard deviations).  The kernel's band sums run at most ceil(nc / 256) + APART terms per thread (from global memory a
          thread takes every 256th candidate of each of the APART parts), 6 shuffle steps and 3 adds:
          n = ceil(nc / 256) + APART + 9; the rank form of typical (nc <= EXACT_CAP) sums nc terms in a row: n = nc.  g = that bound + 2 u
          also covers the product t Z or e Z.
    Z:    [sum over `kept` of p (1 - d), sum over `maybe` of p (1 + d)], widened by g.
    A:    terms p log p <= 0 with |error| <= p (d |log p| + dlog (1 + d)) + 2 u p |log p|; more tokens make A smaller, so the
          lower end sums `maybe` and the upper end `kept`; the sum's own error is g sum |p log p|.
    c, H: from the ends of A and Z (A <= 0 < Z), plus 4 u (1 + |value|) for the division, the logarithm and the subtraction.
    d_i:  the interval of |c - log p_i|; with more than EXACT_CAP candidates the kernel bisects on d in fp32 and probes the
          p-interval [exp(c - d), exp(c + d)]: 2^-21 (1 + |c| + d_i) more (fp32 spacing of d, the two expf and their arguments).
    thresholds e Z and the eta factor: the ends of their inputs, widened by 2 u per operation.
"""
import numpy as np

import oracle.sampling as osamp

U = 2.0 ** -24
WARPERS_OFF = (0.0, 1.0, 0.0, 0.0)


def _f32(x) -> float:
    return float(np.float32(x))


class WarpRef(osamp.HeadRef):
    """HeadRef extended to a band: `kept` / `maybe` are the sets after the warpers, draw() / admissible() work over them.
    `base_kept` / `base_maybe`: what top-k / top-p kept.  `borderline` = maybe & ~kept."""

    def __init__(self, logits, temperature, top_p, top_k=0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
        super().__init__(logits, temperature, top_p, top_k)
        self.base_kept, self.base_maybe = self.kept.copy(), self.maybe.copy()
        l = np.asarray(logits, dtype=np.float32).astype(np.float64)
        ids = np.nonzero(self.maybe)[0]
        self._l, self._p, self._d = l[ids], self.p[ids], self.d[ids]
        self._plo, self._phi = np.maximum(self._p * (1 - self._d), 0.0), self._p * (1 + self._d)
        with np.errstate(divide="ignore"):
            self._lg = np.where(self._p > 0, np.log(np.maximum(self._p, 1e-300)), -np.inf)
        self._dlg = 1.01 * self._d + 4 * U * np.abs(self._lg)
        self.sure, self.may = self.kept[ids].copy(), np.ones(ids.size, dtype=bool)
        self.bisect = self.nc > osamp.EXACT_CAP
        self.g = osamp._sum_margin(-(-self.nc // 256) + osamp.APART + 9) + 2 * U
        self.g_rank = osamp._sum_margin(max(self.nc, 1)) + 2 * U
        m, t, e, h = _f32(min_p), _f32(typical_p), _f32(epsilon_cutoff), _f32(eta_cutoff)
        if m > 0:
            self._narrow(self._plo >= m, self._phi >= m)
        if t < 1:
            self._typical(t)
        if e > 0:
            self._cut(e, e)
        if h > 0:
            H_lo, H_hi = self._entropy()
            self._cut(min(h, np.sqrt(h) * np.exp(-H_hi)) * (1 - 8 * U), min(h, np.sqrt(h) * np.exp(-H_lo)) * (1 + 8 * U))
        self.kept = np.zeros(self.V, dtype=bool)
        self.maybe = np.zeros(self.V, dtype=bool)
        self.kept[ids[self.sure]] = True
        self.maybe[ids[self.may]] = True
        self.borderline = self.maybe & ~self.kept
        self.undecided = int(self.borderline.sum())
        # the draw's CDF bounds over the possibly-kept tokens in index order (HeadRef's, over the narrowed sets)
        ids = np.nonzero(self.maybe)[0]
        mlo, mhi = np.maximum(self.p * (1 - self.d), 0.0), self.p * (1 + self.d)
        self.ids = ids
        self.C_lo = np.cumsum(np.where(self.kept[ids], mlo[ids], 0.0)) * (1 - self.g_draw)
        self.C_hi = np.cumsum(mhi[ids]) * (1 + self.g_draw)
        self.C = np.cumsum(np.where(self.kept[ids], self.p[ids], 0.0))
        self.total_lo, self.total_hi, self.total = self.C_lo[-1], self.C_hi[-1], self.C[-1]

    def _narrow(self, certain, possible):
        self.sure = self.sure & certain
        self.may = self.may & possible
        self.sure &= self.may

    def _Z(self):
        return float(self._plo[self.sure].sum()) * (1 - self.g), float(self._phi[self.may].sum()) * (1 + self.g)

    def _center(self):
        """Ends of c = A / Z over the current band."""
        Z_lo, Z_hi = self._Z()
        with np.errstate(invalid="ignore"):
            term = np.where(self._p > 0, self._p * self._lg, 0.0)                  # <= 0
        err = self._p * (self._d * np.abs(self._lg) + self._dlg * (1 + self._d)) + 2 * U * np.abs(term)
        S = float(np.abs(term[self.may]).sum())
        A_lo = float((term - err)[self.may].sum()) - self.g * S
        A_hi = min(float((term + err)[self.sure].sum()) + self.g * S, 0.0) if self.sure.any() else 0.0
        Z_lo = max(Z_lo, 1e-300)
        c_lo, c_hi = A_lo / Z_lo, A_hi / Z_hi
        return c_lo - 4 * U * (1 + abs(c_lo)), c_hi + 4 * U * (1 + abs(c_hi)), Z_lo, Z_hi

    def _entropy(self):
        c_lo, c_hi, Z_lo, Z_hi = self._center()
        H_lo, H_hi = np.log(Z_lo) - c_hi, np.log(Z_hi) - c_lo
        return H_lo - 4 * U * (1 + abs(H_lo)), H_hi + 4 * U * (1 + abs(H_hi))

    def _typical(self, t):
        c_lo, c_hi, Z_lo, Z_hi = self._center()
        u_lo, u_hi = c_lo - (self._lg + self._dlg), c_hi - (self._lg - self._dlg)   # ends of c - log p_i
        dd_lo = np.where((u_lo <= 0) & (u_hi >= 0), 0.0, np.minimum(np.abs(u_lo), np.abs(u_hi)))
        dd_hi = np.maximum(np.abs(u_lo), np.abs(u_hi))
        if self.bisect:
            s = 2.0 ** -21 * (1 + max(abs(c_lo), abs(c_hi)) + dd_hi)
            dd_lo, dd_hi = np.maximum(dd_lo - s, 0.0), dd_hi + s
        g = self.g if self.bisect else self.g_rank
        need_lo, need_hi = t * Z_lo * (1 - g), t * Z_hi * (1 + g)
        n = self._p.size
        # possibly kept: even the surely-nearer sure tokens at their least stay below the largest t Z
        js = np.nonzero(self.sure)[0]
        o = js[np.argsort(dd_hi[js], kind="stable")]
        cum = np.concatenate([[0.0], np.cumsum(self._plo[o])]) * (1 - g)
        possible = cum[np.searchsorted(dd_hi[o], dd_lo, side="left")] < need_hi
        # surely kept: all possibly-nearer tokens at their most (exact ties of i - the same logit, the same fp32 d - are never
        # strictly nearer) stay below the smallest t Z
        jm = np.nonzero(self.may)[0]
        o = jm[np.argsort(dd_lo[jm], kind="stable")]
        cum = np.concatenate([[0.0], np.cumsum(self._phi[o])]) * (1 + g)
        near = cum[np.searchsorted(dd_lo[o], dd_hi, side="left")]
        _, inv, cnt = np.unique(np.where(self.may, self._l, np.inf), return_inverse=True, return_counts=True)
        ties = np.where(self.may & (dd_lo < dd_hi), cnt[inv] * self._phi * (1 + g), 0.0)
        certain = (near - ties) < need_lo
        self._narrow(certain, possible)

    def _cut(self, e_lo, e_hi):
        """keep p >= min(e Z, max p), e in [e_lo, e_hi]."""
        Z_lo, Z_hi = self._Z()
        top_may = float(self._phi[self.may].max())
        top_sure = float(self._plo[self.sure].max()) if self.sure.any() else 0.0
        thr_hi = min(e_hi * Z_hi * (1 + 2 * U), top_may)
        thr_lo = min(e_lo * Z_lo * (1 - 2 * U), top_sure)
        l_top = self._l[self.may].max()
        self._narrow((self._plo >= thr_hi) | (self._l >= l_top), self._phi >= thr_lo)


# ------------------------------------------------------------------------------------------------ the draw matrix
def rows(kind, V, B, seed):
    """fp32 logits [B, V] of one row kind (the kinds of the sampling head's own draw matrix)."""
    r = np.random.default_rng(seed)
    if kind.startswith("gauss"):
        x = r.standard_normal((B, V)) * float(kind[5:])
    elif kind == "peaked":                                  # one logit far above the rest
        x = r.standard_normal((B, V)) * 2.0
        x[np.arange(B), r.integers(0, V, B)] += 12.0
    elif kind == "flat":                                    # all equal: p = 1 exactly, every sum exact
        x = np.zeros((B, V))
    elif kind == "tie50":                                   # the 50th value tied three more times
        x = r.standard_normal((B, V)) * 2.0
        for b in range(B):
            o = np.argsort(-x[b])
            x[b, o[50:53]] = x[b, o[49]]
    elif kind == "neginf":                                  # -inf entries, and whole parts of them
        x = r.standard_normal((B, V)) * 2.0
        x[r.random((B, V)) < 0.3] = -np.inf
        x[:, : int(0.4 * V)] = -np.inf
    elif kind == "pm1e4":                                   # rows near +1e4 and -1e4
        x = r.standard_normal((B, V)) + np.where(np.arange(B) % 2 == 0, 1e4, -1e4)[:, None]
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


ALL4 = (0.02, 0.9, 3e-4, 3e-4)
# (V, rows = max_batch, row kind, temperature, top_p, top_k, (min_p, typical_p, epsilon_cutoff, eta_cutoff), steps, what it is for)
MATRIX = [
    (96, 8, "gauss2", 1.0, 1.0, 0, (0.05, 1.0, 0.0, 0.0), 128, "min_p alone"),
    (96, 8, "gauss1", 1.0, 1.0, 0, (0.0, 0.2, 0.0, 0.0), 128, "typical alone, arg-max dropped"),
    (96, 8, "peaked", 1.0, 1.0, 0, (0.0, 1.0, 0.01, 0.0), 128, "epsilon alone"),
    (96, 8, "tie50", 1.0, 1.0, 0, (0.0, 1.0, 0.0, 0.02), 128, "eta alone, tied values"),
    (96, 8, "gauss2", 1.0, 0.9, 50, ALL4, 128, "all four behind top-k 50 / top-p 0.9"),
    (1040, 128, "gauss1", 1.0, 1.0, 0, (0.0, 0.2, 0.0, 0.0), 16, "typical by bisection in LDS, arg-max dropped"),
    (1040, 128, "neginf", 1.0, 0.9, 50, ALL4, 16, "all four, -inf entries"),
    (1040, 128, "flat", 0.7, 1.0, 0, (0.0, 1.0, 0.002, 0.0), 16, "epsilon > 1 / V on equal values: nothing removed"),
    (1040, 128, "gauss2", 2.0, 1.0, 0, (0.1, 0.8, 1e-3, 2e-3), 16, "all four in LDS"),
    (32000, 16, "gauss4", 1.0, 1.0, 0, (0.05, 1.0, 0.0, 0.0), 64, "min_p from global memory"),
    (32000, 16, "gauss2", 1.0, 0.9, 50, ALL4, 64, "all four behind top-k 50 / top-p 0.9"),
    (32000, 16, "gauss2", 0.4, 0.9, 0, (0.0, 0.7, 0.0, 1e-3), 64, "typical + eta, a few thousand candidates"),
    (128256, 16, "gauss4", 1.0, 1.0, 0, (0.0, 0.3, 0.0, 0.0), 64, "typical by bisection from global memory, arg-max dropped"),
    (128256, 16, "flat", 1.0, 1.0, 0, (0.0, 0.5, 0.0, 0.0), 64, "typical on equal values: one tie, all kept"),
    (128256, 16, "gauss4", 1.0, 1.0, 0, (0.0, 1.0, 1e-4, 1e-3), 64, "epsilon + eta from global memory"),
    (1040, 128, "pm1e4", 0.1, 0.7, 50, (0.02, 0.5, 3e-4, 3e-4), 16, "all four on rows near +-1e4 (p rounds by 2.4e-2 at temperature 0.1)"),
    (128256, 16, "pm1e4", 0.1, 0.7, 50, (0.0, 0.5, 0.0, 1e-3), 64, "typical + eta on rows near +-1e4"),
]
NONDECISIVE_MAX = 0.02        # per case (the sampling head's own cap)
NONDECISIVE_MAX_PM1E4 = 0.10  # rows near +-1e4: the exponent's fp32 rounding, 2^-23 (|l| + |max|) / T, is 2.4e-2 at temperature 0.1


def nondecisive_cap(kind):
    return NONDECISIVE_MAX_PM1E4 if kind == "pm1e4" else NONDECISIVE_MAX
SEED = 0x5EED


def branch(nc):
    return "exact" if nc <= osamp.EXACT_CAP else ("lds" if nc <= osamp.LDS_CAP else "global")


_CASE_CACHE = {}


def case_refs(i):
    """(logits, [WarpRef per row], per row (pick, decisive, lowest id, highest id) over the case's steps) of MATRIX[i], computed once."""
    if i not in _CASE_CACHE:
        V, B, kind, T, tp, k, w, steps, _ = MATRIX[i]
        logits = rows(kind, V, B, V + len(kind))
        refs = [WarpRef(logits[b], T, tp, k, *w) for b in range(B)]
        draws = [refs[b].draw(np.array([osamp.draw_uniform(SEED, b, s)[1] for s in range(steps)])) for b in range(B)]
        _CASE_CACHE[i] = (logits, refs, draws)
    return _CASE_CACHE[i]
