// Attention of NEW rows over a cached prefix, in two forms of one kernel: attn_prefix_kernel<HD, TREE>.
//
// Flat form (TREE = false, opus_llama_score_continuations): the queries are continuation rows of n positions each.
//   continuation row r (prefix row p = src[r], n positions, query t):
//     keys = cache slots kstart[p] .. Tp - 1 of row p (K rotated when the prefix was prefilled)
//          + the row's own positions 0 .. t (causal; projections rotated by the caller at positions Tp - kstart[p] + t)
//
// Tree form (TREE = true, opus_llama_score_tree; selected by AttnPrefixParams::par): every row is ONE new position (n = 1, fixed
// at compile time), a node of a token trie behind the cached prompt.
//   row r (prefix row p = src[r], parent row par[r] of the same pass or -1 for a child of the root):
//     keys = cache slots kstart[p] .. Tp - 1 of row p
//          + rows r, par[r], par[par[r]], ... of this pass's projections (rotated by the caller at Tp - kstart[p] + depth - 1)
//
// Work split.  One workgroup per (prefix row p, kv head hk, block of 128 stacked queries).  The queries of a prefix row are
// STACKED: every row i of p (the rows src maps to p, in the order of the list), every head of the GQA group and every
// position t form one index q = (i G + gh) n + t.  The prefix's K / V tiles are then read once per (p, hk) and query block and
// shared by all K continuations and all G heads of the group (K options x 4 heads x 6 positions = 96 queries: one workgroup),
// instead of once per continuation row and head.  In the flat form the own-position keys of a block are the n positions of the
// continuations the block's queries belong to (a block-diagonal causal mask over that short virtual key list), tiled like the
// cache part.
//
// In the tree form the ancestor part is not tiled: a query has at most `depth` such keys and no two queries of a block need
// share any, so a virtual key list of the block would cost every query the block's whole list.  Instead each query walks its
// own parent chain after the cache part: the four lanes (li, g = 0 .. 3) that hold a query take 8 dims of each 32-dim step of
// q . k (the MFMA B-fragment they already hold), two xor-shuffles complete the score, and every lane updates the 4 output dims
// per 16-dim tile that it owns in the MFMA result layout.  The cost per query is its own depth, whatever else the pass holds.
// The chain is walked from the node up to the root in a fixed order, so the same inputs give bitwise the same output.
//
// Per wave 32 queries (two 16-query tiles, QT = 2); 64-key tiles staged in LDS (K row-major, V transposed so that the P V
// product reads V^T rows as 8-byte pieces).  The products are swapped, as in attn_prefill.hip, so that a query lives on a lane:
//   S^T = K Q^T   MFMA 16x16x32 (A = 16 keys x 32 dims from LDS, B = Q^T from registers): lane (li = query, g) holds the
//                 scores of its query for keys 16 n + 4 g + r
//   O^T += V^T P^T  the probabilities as they stand are the B operand of a 32-key step (contraction index 8 g + e = key
//                 16 (2 j + e / 4) + 4 g + e % 4), the A operand takes V^T[dim][the same keys] from the transposed image.
// Online softmax in base 2, fp32 throughout; the output is normalised and stored in the operand dtype [R n, heads hd].
#include "common.h"

namespace opus {

namespace {

constexpr int PKB = 64;            // keys per tile
constexpr int PQT = 2;             // 16-query tiles per wave
constexpr int PQB = 4 * 16 * PQT;  // queries per workgroup
constexpr int VT_PAD = 8;          // halfs of padding behind each row of the transposed V image (row pitch 72: 144 B)

template <int HD, bool TREE>
__global__ __launch_bounds__(256) void attn_prefix_kernel(AttnPrefixParams p) {
    constexpr int KS = HD < 32 ? 1 : HD / 32;   // MFMA k-steps of QK^T (head_dim 16: one step, upper half zero)
    constexpr int NO = HD / 16;                 // output dim tiles
    constexpr int VC = HD / 8;                  // 16-B chunks per K / V row
    constexpr int VTP = PKB + VT_PAD;
    __shared__ __attribute__((aligned(16))) half_t sK[PKB * HD];
    __shared__ __attribute__((aligned(16))) half_t sVt[HD * VTP];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int pr = p.blocks[2 * blockIdx.x], q0 = p.blocks[2 * blockIdx.x + 1];
    const int hk = blockIdx.y;
    const int G = p.nh / p.nkv, n = TREE ? 1 : p.n, Gn = G * n;   // (TREE: the divisions by n fold)
    const int lo = p.off[pr], cnt = p.off[pr + 1] - lo;
    const int nq = cnt * Gn;                                    // stacked queries of this prefix row
    const int QKV = (p.nh + 2 * p.nkv) * HD, QD = p.nh * HD;
    const int kbeg = p.kstart[pr], Lp = p.Tp - kbeg;           // visible cache slots kbeg .. Tp - 1
    // own-position keys of the block (flat form): the n positions of continuations i_lo .. i_hi
    const int qlast = (q0 + PQB < nq ? q0 + PQB : nq) - 1;
    const int i_lo = q0 / Gn, i_hi = qlast / Gn;
    const int nself = (i_hi - i_lo + 1) * n;

    const half_t *kc = p.kc + (int64_t)pr * p.cache_sb + (int64_t)hk * p.cache_sh;
    const half_t *vc = p.vc + (int64_t)pr * p.cache_sb + (int64_t)hk * p.cache_sh;

    // this lane's queries: (row i, head gh, position t) -> Q row; flat form: the own-key window [jlo, jhi] of the virtual list,
    // tree form: the node's row of the pass
    h8 qf[PQT][KS];
    int jlo[PQT], jhi[PQT], qrow[PQT];
    int64_t orow[PQT];
    bool qok[PQT];
#pragma unroll
    for (int u = 0; u < PQT; ++u) {
        int q = q0 + wave * 16 * PQT + 16 * u + li;
        qok[u] = q < nq;
        q = qok[u] ? q : nq - 1;
        const int i = q / Gn, rem = q - i * Gn, gh = rem / n, t = rem - gh * n;
        const int r = p.list[lo + i];
        const int64_t row = (int64_t)r * n + t;
        const half_t *src = p.qkv + row * QKV + (int64_t)(hk * G + gh) * HD;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int d = 32 * s + 8 * g;
            qf[u][s] = d < HD ? *reinterpret_cast<const h8 *>(src + d) : h8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        jlo[u] = (i - i_lo) * n;
        jhi[u] = jlo[u] + t;
        qrow[u] = r;
        orow[u] = row * QD + (int64_t)(hk * G + gh) * HD;
    }
    const bool wave_live = q0 + wave * 16 * PQT < nq;          // (wave-uniform)

    f4 o[PQT][NO];
    float mrow[PQT], lrow[PQT];
#pragma unroll
    for (int u = 0; u < PQT; ++u) {
        mrow[u] = -INFINITY;
        lrow[u] = 0.f;
#pragma unroll
        for (int d = 0; d < NO; ++d) o[u][d] = f4{0.f, 0.f, 0.f, 0.f};
    }
    const float sc = p.scale * 1.4426950408889634f;

    // stage keys kt .. kt + 63 of part `self` (0: cache slots kbeg + j, 1: own positions j) into LDS; keys past the end are zeros
    auto stage = [&](int self, int kt, int nk) {
        for (int e = tid; e < PKB * VC; e += 256) {
            const int rr = e / VC, c = e - rr * VC, j = kt + rr;
            h8 kv = h8{0, 0, 0, 0, 0, 0, 0, 0}, vv = kv;
            if (j < nk) {
                const half_t *ks, *vs;
                if (!self) {
                    ks = kc + (int64_t)(kbeg + j) * HD;
                    vs = vc + (int64_t)(kbeg + j) * HD;
                } else {
                    const int ik = j / n, tk = j - ik * n;
                    const int64_t row = (int64_t)p.list[lo + i_lo + ik] * n + tk;
                    ks = p.qkv + row * QKV + QD + (int64_t)hk * HD;
                    vs = ks + (int64_t)p.nkv * HD;
                }
                kv = *reinterpret_cast<const h8 *>(ks + c * 8);
                vv = *reinterpret_cast<const h8 *>(vs + c * 8);
            }
            *reinterpret_cast<h8 *>(&sK[rr * HD + c * 8]) = kv;
#pragma unroll
            for (int x = 0; x < 8; ++x) sVt[(c * 8 + x) * VTP + rr] = vv[x];
        }
    };

    auto tile = [&](int self, int kt, int nk) {
        f4 s[PQT][4];
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) {
            const int r = 16 * nn + li;
            h8 kf[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int d = 32 * ks + 8 * g;
                kf[ks] = d < HD ? *reinterpret_cast<const h8 *>(&sK[r * HD + d]) : h8{0, 0, 0, 0, 0, 0, 0, 0};
            }
#pragma unroll
            for (int u = 0; u < PQT; ++u) {
                s[u][nn] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s[u][nn] = mfma16(kf[ks], qf[u][ks], s[u][nn]);
            }
        }
        // masks: cache part - keys past the prefix end; own part - the window of this query's continuation, causal
        const bool full = !self && kt + PKB <= nk;
        if (!full) {
#pragma unroll
            for (int u = 0; u < PQT; ++u)
#pragma unroll
                for (int nn = 0; nn < 4; ++nn)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = kt + 16 * nn + 4 * g + r;
                        const bool vis = self ? (j >= jlo[u] && j <= jhi[u]) : j < nk;
                        s[u][nn][r] = vis ? s[u][nn][r] : -INFINITY;
                    }
        }
        h8 pf[PQT][2];
#pragma unroll
        for (int u = 0; u < PQT; ++u) {
            float mx = s[u][0][0];
#pragma unroll
            for (int nn = 0; nn < 4; ++nn)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[u][nn][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mnew = fmaxf(mrow[u], mx);
            const float msafe = mnew == -INFINITY ? 0.f : mnew;      // (no visible key so far)
            if (!__all(mnew == mrow[u])) {
                const float alpha = __builtin_amdgcn_exp2f((mrow[u] - msafe) * sc);   // 0 when mrow = -inf
                lrow[u] *= alpha;
#pragma unroll
                for (int d = 0; d < NO; ++d) o[u][d] *= alpha;
                mrow[u] = mnew;
            }
            const float msc = msafe * sc;
            float rs = 0.f;
#pragma unroll
            for (int nn = 0; nn < 4; ++nn)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __builtin_amdgcn_exp2f(s[u][nn][r] * sc - msc);
                    s[u][nn][r] = e;
                    rs += e;
                }
            lrow[u] += rs;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                pf[u][j] = h8{(half_t)s[u][2 * j][0], (half_t)s[u][2 * j][1], (half_t)s[u][2 * j][2], (half_t)s[u][2 * j][3],
                              (half_t)s[u][2 * j + 1][0], (half_t)s[u][2 * j + 1][1], (half_t)s[u][2 * j + 1][2],
                              (half_t)s[u][2 * j + 1][3]};
        }
        // O^T += V^T P^T: lane (li, g) of dim tile d takes V^T[16 d + li][32 j + 4 g + 0..3] and [32 j + 16 + 4 g + 0..3]
#pragma unroll
        for (int d = 0; d < NO; ++d)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const half_t *vr = &sVt[(16 * d + li) * VTP + 32 * j + 4 * g];
                const h4 a = *reinterpret_cast<const h4 *>(vr);
                const h4 b = *reinterpret_cast<const h4 *>(vr + 16);
                const h8 vf = h8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
                for (int u = 0; u < PQT; ++u) o[u][d] = mfma16(vf, pf[u][j], o[u][d]);
            }
    };

    for (int self = 0; self < (TREE ? 1 : 2); ++self) {            // (the tree form has no tiled own part)
        const int nk = self ? nself : Lp;
        for (int kt = 0; kt < nk; kt += PKB) {
            __syncthreads();                                        // (the previous tile's readers are done)
            stage(self, kt, nk);
            __syncthreads();
            if (wave_live) tile(self, kt, nk);
        }
    }

    if (!wave_live) return;

    if constexpr (TREE) {
        // the node and its ancestors: one key per step and query, walked up the parent chain (lanes past the end repeat the
        // block's last query, so every lane of the wave holds a valid chain; a finished chain idles at cur = -1)
        int cur[PQT];
#pragma unroll
        for (int u = 0; u < PQT; ++u) cur[u] = qrow[u];
        while (__any(cur[0] >= 0 || cur[1] >= 0)) {
#pragma unroll
            for (int u = 0; u < PQT; ++u) {
                const bool act = cur[u] >= 0;
                const int kr = act ? cur[u] : qrow[u];
                const half_t *kp = p.qkv + (int64_t)kr * QKV + QD + (int64_t)hk * HD;
                const half_t *vp = kp + (int64_t)p.nkv * HD;
                float dot = 0.f;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const int d = 32 * s + 8 * g;
                    if (d < HD) {
                        const h8 kf = *reinterpret_cast<const h8 *>(kp + d);
#pragma unroll
                        for (int x = 0; x < 8; ++x) dot = fmaf((float)qf[u][s][x], (float)kf[x], dot);
                    }
                }
                dot += __shfl_xor(dot, 16, 64);
                dot += __shfl_xor(dot, 32, 64);
                const float sv = act ? dot : -INFINITY;
                const float mnew = fmaxf(mrow[u], sv);
                const float msafe = mnew == -INFINITY ? 0.f : mnew;
                const float alpha = __builtin_amdgcn_exp2f((mrow[u] - msafe) * sc);       // 1 when the maximum stays, 0 from -inf
                const float pe = act ? __builtin_amdgcn_exp2f((sv - msafe) * sc) : 0.f;
                lrow[u] = lrow[u] * alpha + (g == 0 ? pe : 0.f);      // (lrow is a per-lane partial: the key counts once)
                mrow[u] = mnew;
#pragma unroll
                for (int d = 0; d < NO; ++d) {
                    const h4 vv = *reinterpret_cast<const h4 *>(vp + 16 * d + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[u][d][r] = fmaf(pe, (float)vv[r], o[u][d][r] * alpha);
                }
                cur[u] = act ? p.par[kr] : -1;
            }
        }
    }

#pragma unroll
    for (int u = 0; u < PQT; ++u) {
        float l = lrow[u];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        if (!qok[u]) continue;
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        half_t *dst = p.out + orow[u];
#pragma unroll
        for (int d = 0; d < NO; ++d)
            *reinterpret_cast<h4 *>(dst + 16 * d + 4 * g) =
                h4{(half_t)(o[u][d][0] * inv), (half_t)(o[u][d][1] * inv), (half_t)(o[u][d][2] * inv), (half_t)(o[u][d][3] * inv)};
    }
}

}  // namespace

int attn_prefix_blocks(const int32_t *off, int P, int G, int n, int32_t *blocks) {
    int nb = 0;
    for (int pr = 0; pr < P; ++pr) {
        const int nq = (off[pr + 1] - off[pr]) * G * n;
        for (int q0 = 0; q0 < nq; q0 += PQB) {
            if (blocks) {
                blocks[2 * nb] = pr;
                blocks[2 * nb + 1] = q0;
            }
            ++nb;
        }
    }
    return nb;
}

int attn_prefix_max_blocks(int R, int P, int G, int n) { return (int)(((int64_t)R * G * n) / PQB) + P; }

template <bool TREE>
static hipError_t launch_form(const AttnPrefixParams &p, dim3 grid, hipStream_t s) {
    switch (p.hd) {
        case 16: OPUS_LAUNCH(KC_ATTN_PREFILL, (attn_prefix_kernel<16, TREE>), grid, dim3(256), 0, s, p); break;
        case 32: OPUS_LAUNCH(KC_ATTN_PREFILL, (attn_prefix_kernel<32, TREE>), grid, dim3(256), 0, s, p); break;
        case 64: OPUS_LAUNCH(KC_ATTN_PREFILL, (attn_prefix_kernel<64, TREE>), grid, dim3(256), 0, s, p); break;
        case 128: OPUS_LAUNCH(KC_ATTN_PREFILL, (attn_prefix_kernel<128, TREE>), grid, dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_attn_prefix(const AttnPrefixParams &p, int nblocks, hipStream_t s) {
    if (nblocks <= 0) return hipSuccess;
    const bool tree = p.par != nullptr;                         // (the tree form: one position per row)
    if (p.nkv < 1 || p.nh % p.nkv || p.n < 1 || p.Tp < 1 || (tree && p.n != 1)) return hipErrorInvalidValue;
    const dim3 grid(nblocks, p.nkv);
    return tree ? launch_form<true>(p, grid, s) : launch_form<false>(p, grid, s);
}

}  // namespace opus
