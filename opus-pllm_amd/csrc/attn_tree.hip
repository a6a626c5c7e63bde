// Tree attention of opus_llama_score_tree: every query is ONE new position (a node of a token trie behind a cached prompt), the
// keys are the cached prompt plus the node's ancestors and the node itself.
//
//   row r (prefix row p = src[r], parent row par[r] of the same pass or -1 for a child of the root):
//     keys = cache slots kstart[p] .. Tp - 1 of row p (K rotated when the prompt was prefilled)
//          + rows r, par[r], par[par[r]], ... of this pass's projections (rotated by the caller at Tp - kstart[p] + depth - 1)
//
// Work split, as attn_prefix_kernel with n = 1: one workgroup per (prefix row p, kv head hk, block of 128 stacked queries), the
// stacked index of node i of p (position in the list) and head gh of the GQA group being q = i G + gh.  The prefix's K / V tiles
// are staged in LDS once per block and shared by its 128 queries (swapped MFMA products, online softmax in base 2, fp32; the
// layout comments of attn_prefix.hip apply word for word).
//
// The ancestor part is not tiled: a query has at most `depth` such keys and no two queries of a block need share any, so a
// virtual key list of the block would cost every query the block's whole list.  Instead each query walks its own parent chain:
// the four lanes (li, g = 0 .. 3) that hold a query take 8 dims of each 32-dim step of q . k (the MFMA B-fragment they already
// hold), two xor-shuffles complete the score, and every lane updates the 4 output dims per 16-dim tile that it owns in the
// MFMA result layout.  The cost per query is its own depth, whatever else the pass holds.  The chain is walked from the node up
// to the root in a fixed order, so the same inputs give bitwise the same output.
#include "common.h"

namespace opus {

namespace {

constexpr int TKB = 64;            // keys per tile
constexpr int TQT = 2;             // 16-query tiles per wave
constexpr int TQB = 4 * 16 * TQT;  // queries per workgroup (= attn_prefix_kernel's: the workgroup table is attn_prefix_blocks(n = 1))
constexpr int TVT_PAD = 8;         // halfs of padding behind each row of the transposed V image

template <int HD>
__global__ __launch_bounds__(256) void attn_tree_kernel(AttnPrefixParams p) {
    constexpr int KS = HD < 32 ? 1 : HD / 32;   // MFMA k-steps of QK^T (head_dim 16: one step, upper half zero)
    constexpr int NO = HD / 16;                 // output dim tiles
    constexpr int VC = HD / 8;                  // 16-B chunks per K / V row
    constexpr int VTP = TKB + TVT_PAD;
    __shared__ __attribute__((aligned(16))) half_t sK[TKB * HD];
    __shared__ __attribute__((aligned(16))) half_t sVt[HD * VTP];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    const int pr = p.blocks[2 * blockIdx.x], q0 = p.blocks[2 * blockIdx.x + 1];
    const int hk = blockIdx.y;
    const int G = p.nh / p.nkv;
    const int lo = p.off[pr], cnt = p.off[pr + 1] - lo;
    const int nq = cnt * G;                                     // stacked queries of this prefix row
    const int QKV = (p.nh + 2 * p.nkv) * HD, QD = p.nh * HD;
    const int kbeg = p.kstart[pr], Lp = p.Tp - kbeg;           // visible cache slots kbeg .. Tp - 1

    const half_t *kc = p.kc + (int64_t)pr * p.cache_sb + (int64_t)hk * p.cache_sh;
    const half_t *vc = p.vc + (int64_t)pr * p.cache_sb + (int64_t)hk * p.cache_sh;

    // this lane's queries: (node i, head gh) -> its row of the pass
    h8 qf[TQT][KS];
    int qrow[TQT];
    int64_t orow[TQT];
    bool qok[TQT];
#pragma unroll
    for (int u = 0; u < TQT; ++u) {
        int q = q0 + wave * 16 * TQT + 16 * u + li;
        qok[u] = q < nq;
        q = qok[u] ? q : nq - 1;
        const int i = q / G, gh = q - i * G;
        const int r = p.list[lo + i];
        const half_t *src = p.qkv + (int64_t)r * QKV + (int64_t)(hk * G + gh) * HD;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int d = 32 * s + 8 * g;
            qf[u][s] = d < HD ? *reinterpret_cast<const h8 *>(src + d) : h8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        qrow[u] = r;
        orow[u] = (int64_t)r * QD + (int64_t)(hk * G + gh) * HD;
    }
    const bool wave_live = q0 + wave * 16 * TQT < nq;          // (wave-uniform)

    f4 o[TQT][NO];
    float mrow[TQT], lrow[TQT];
#pragma unroll
    for (int u = 0; u < TQT; ++u) {
        mrow[u] = -INFINITY;
        lrow[u] = 0.f;
#pragma unroll
        for (int d = 0; d < NO; ++d) o[u][d] = f4{0.f, 0.f, 0.f, 0.f};
    }
    const float sc = p.scale * 1.4426950408889634f;

    // stage cache slots kbeg + kt .. kbeg + kt + 63 into LDS; slots past the prefix end are zeros
    auto stage = [&](int kt) {
        for (int e = tid; e < TKB * VC; e += 256) {
            const int rr = e / VC, c = e - rr * VC, j = kt + rr;
            h8 kv = h8{0, 0, 0, 0, 0, 0, 0, 0}, vv = kv;
            if (j < Lp) {
                kv = *reinterpret_cast<const h8 *>(kc + (int64_t)(kbeg + j) * HD + c * 8);
                vv = *reinterpret_cast<const h8 *>(vc + (int64_t)(kbeg + j) * HD + c * 8);
            }
            *reinterpret_cast<h8 *>(&sK[rr * HD + c * 8]) = kv;
#pragma unroll
            for (int x = 0; x < 8; ++x) sVt[(c * 8 + x) * VTP + rr] = vv[x];
        }
    };

    auto tile = [&](int kt) {
        f4 s[TQT][4];
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
            for (int u = 0; u < TQT; ++u) {
                s[u][nn] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s[u][nn] = mfma16(kf[ks], qf[u][ks], s[u][nn]);
            }
        }
        if (kt + TKB > Lp) {                                       // keys past the prefix end
#pragma unroll
            for (int u = 0; u < TQT; ++u)
#pragma unroll
                for (int nn = 0; nn < 4; ++nn)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = kt + 16 * nn + 4 * g + r;
                        s[u][nn][r] = j < Lp ? s[u][nn][r] : -INFINITY;
                    }
        }
        h8 pf[TQT][2];
#pragma unroll
        for (int u = 0; u < TQT; ++u) {
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
#pragma unroll
        for (int d = 0; d < NO; ++d)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const half_t *vr = &sVt[(16 * d + li) * VTP + 32 * j + 4 * g];
                const h4 a = *reinterpret_cast<const h4 *>(vr);
                const h4 b = *reinterpret_cast<const h4 *>(vr + 16);
                const h8 vf = h8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
                for (int u = 0; u < TQT; ++u) o[u][d] = mfma16(vf, pf[u][j], o[u][d]);
            }
    };

    for (int kt = 0; kt < Lp; kt += TKB) {
        __syncthreads();                                            // (the previous tile's readers are done)
        stage(kt);
        __syncthreads();
        if (wave_live) tile(kt);
    }
    if (!wave_live) return;

    // the node and its ancestors: one key per step and query, walked up the parent chain (lanes past the end repeat the
    // block's last query, so every lane of the wave holds a valid chain; a finished chain idles at cur = -1)
    int cur[TQT];
#pragma unroll
    for (int u = 0; u < TQT; ++u) cur[u] = qrow[u];
    while (__any(cur[0] >= 0 || cur[1] >= 0)) {
#pragma unroll
        for (int u = 0; u < TQT; ++u) {
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

#pragma unroll
    for (int u = 0; u < TQT; ++u) {
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

hipError_t launch_attn_tree(const AttnPrefixParams &p, int nblocks, hipStream_t s) {
    if (nblocks <= 0) return hipSuccess;
    if (p.nkv < 1 || p.nh % p.nkv || p.n != 1 || p.Tp < 1 || !p.par) return hipErrorInvalidValue;
    const dim3 grid(nblocks, p.nkv);
    switch (p.hd) {
        case 16: OPUS_LAUNCH(KC_ATTN_PREFILL, attn_tree_kernel<16>, grid, dim3(256), 0, s, p); break;
        case 32: OPUS_LAUNCH(KC_ATTN_PREFILL, attn_tree_kernel<32>, grid, dim3(256), 0, s, p); break;
        case 64: OPUS_LAUNCH(KC_ATTN_PREFILL, attn_tree_kernel<64>, grid, dim3(256), 0, s, p); break;
        case 128: OPUS_LAUNCH(KC_ATTN_PREFILL, attn_tree_kernel<128>, grid, dim3(256), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace opus
