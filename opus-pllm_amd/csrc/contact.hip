// ESM-2 contact maps (opus_esm2_contacts_packed): the logistic regression of EsmContactPredictionHead over the symmetrised,
// average-product-corrected attention maps of every layer and head, without ever holding those maps.
//
// For the interior positions i, j (residues, <cls> and <eos> dropped) of one protein and P_c the softmax of channel c = l H + h
// restricted to them (the softmax itself runs over every key of the protein):
//   A      = sum_c w_c P_c                                 accumulated layer by layer (esm_contact_accum_kernel)
//   a_c[i] = sum_j P_c[i, j] + sum_j P_c[j, i]             row sums (accum kernel) + column sums (partials, colsum kernel)
//   s_c    = sum_i a_c[i]                                  (scale kernel: sw_c = w_c / s_c)
//   logit  = bias + A + A^T - sum_c sw_c a_c a_c^T         (finish kernel, exact fp32), contact = sigmoid(logit)
// Every reduction runs in a fixed order and nothing is added atomically: a repeated call is bitwise identical.
//
// Packed layouts (n_b = T_b - 2 interior positions of protein b, its token rows cu[b] .. cu[b + 1] - 1):
//   A / contacts : protein b's [n_b, n_b] block at sum_{b' < b} n_{b'}^2 (row-major)
//   vec          : [sum n_b][C] - row i of protein b at cu[b] - 2 b + i; first the row sums, then a_c
//   part         : [H][sum_b cdiv(n_b, 64) n_b] column-sum partials of one layer: protein b at H sum_{b'<b} cdiv(n_b', 64) n_b',
//                  within it [query block][head][n_b]
#include "common.h"

namespace opus {

constexpr int CQ = 64;          // query rows per workgroup (4 waves x 16) = keys per tile

__device__ __forceinline__ void contact_offsets(const int32_t *cu, int b, int64_t &aoff, int64_t &poff) {
    aoff = 0;
    poff = 0;
    for (int i = 0; i < b; ++i) {
        int n = cu[i + 1] - cu[i] - 2;
        n = n > 0 ? n : 0;
        aoff += (int64_t)n * n;
        poff += (int64_t)((n + CQ - 1) / CQ) * n;
    }
}

// S^T tile of 64 keys x 16 queries: lane (li, g) gets the scores of query li for keys kt + 16 n + 4 g + r (r < 4), keys >= T -> -inf
template <int HD>
__device__ __forceinline__ void contact_scores(const half_t *Kh, int64_t ld, int kt, int T, const h8 *qf, int li, int g, f4 *s) {
    constexpr int HDP = HD < 32 ? 32 : HD, KS = HDP / 32;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        int kr = kt + 16 * n + li;
        kr = kr < T ? kr : T - 1;
        s[n] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int d = 32 * ks + 8 * g;
            const h8 kf = d < HD ? *reinterpret_cast<const h8 *>(Kh + (int64_t)kr * ld + d) : h8{0, 0, 0, 0, 0, 0, 0, 0};
            s[n] = mfma16(kf, qf[ks], s[n]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) s[n][r] = kt + 16 * n + 4 * g + r < T ? s[n][r] : -INFINITY;
    }
}

template <int HD>
__device__ __forceinline__ void contact_q(const half_t *Qh, int64_t ld, int qrow, int g, h8 *qf) {
    constexpr int HDP = HD < 32 ? 32 : HD, KS = HDP / 32;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int d = 32 * ks + 8 * g;
        qf[ks] = d < HD ? *reinterpret_cast<const h8 *>(Qh + (int64_t)qrow * ld + d) : h8{0, 0, 0, 0, 0, 0, 0, 0};
    }
}

// One workgroup per (64 interior query rows, protein), all heads of the layer.  Pass 1: row max and sum of every head over
// every key (<cls> and <eos> included).  Pass 2, per 64-key tile: P of every head recomputed, w_h P summed into the A tile in
// registers, row sums kept in LDS, column sums reduced over the 16 queries of a wave (shuffles) and the 4 waves (LDS).
template <int HD>
__global__ __launch_bounds__(256) void esm_contact_accum_kernel(ContactParams p) {
    constexpr int HDP = HD < 32 ? 32 : HD, KS = HDP / 32;
    extern __shared__ float lds[];
    const int nh = p.heads;
    float *s_m = lds, *s_il = s_m + nh * CQ, *s_rs = s_il + nh * CQ, *s_cs = s_rs + nh * CQ;   // s_cs: [nh][4][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int b = blockIdx.y, qb = blockIdx.x;
    const int r0 = p.cu[b], T = p.cu[b + 1] - r0, nn = T - 2;
    if (nn <= 0 || qb * CQ >= nn) return;                            // (uniform)
    int64_t aoff, poff;
    contact_offsets(p.cu, b, aoff, poff);
    const int64_t voff = r0 - 2 * b;
    const int qi = 1 + qb * CQ + wave * 16 + li;                      // this lane's query token
    const bool qin = qi <= nn;
    const int qrow = qin ? qi : T - 1;
    const int slot = wave * 16 + li;
    for (int i = tid; i < nh * CQ; i += 256) s_rs[i] = 0.f;

    // ---- pass 1: (max, 1 / sum) per query row and head ----
    for (int h = 0; h < nh; ++h) {
        h8 qf[KS];
        contact_q<HD>(p.Q + (int64_t)r0 * p.ld + h * HD, p.ld, qrow, g, qf);
        const half_t *Kh = p.K + (int64_t)r0 * p.ld + h * HD;
        float m = -INFINITY, l = 0.f;
        for (int kt = 0; kt < T; kt += CQ) {
            f4 s[4];
            contact_scores<HD>(Kh, p.ld, kt, T, qf, li, g, s);
            float mt = -INFINITY;
#pragma unroll
            for (int n = 0; n < 4; ++n) mt = fmaxf(fmaxf(mt, fmaxf(s[n][0], s[n][1])), fmaxf(s[n][2], s[n][3]));
            const float mn = fmaxf(m, mt);
            if (mn == -INFINITY) continue;                            // (none of this lane's keys exist yet)
            l = m == -INFINITY ? 0.f : l * __expf(m - mn);
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) l += __expf(s[n][r] - mn);
            m = mn;
        }
        // combine the four key groups (lanes li + 16 g); both lanes of a pair compute the same sum
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
            const float M = fmaxf(m, mo);
            l = (m == -INFINITY ? 0.f : l * __expf(m - M)) + (mo == -INFINITY ? 0.f : lo * __expf(mo - M));
            m = M;
        }
        if (g == 0) {
            s_m[h * CQ + slot] = m;
            s_il[h * CQ + slot] = 1.0f / l;
        }
    }
    __syncthreads();

    // ---- pass 2: interior key tiles ----
    for (int kt = 0; kt <= nn; kt += CQ) {
        f4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = f4{0.f, 0.f, 0.f, 0.f};
        for (int h = 0; h < nh; ++h) {
            h8 qf[KS];
            contact_q<HD>(p.Q + (int64_t)r0 * p.ld + h * HD, p.ld, qrow, g, qf);
            f4 s[4];
            contact_scores<HD>(p.K + (int64_t)r0 * p.ld + h * HD, p.ld, kt, T, qf, li, g, s);
            const float m = s_m[h * CQ + slot], il = s_il[h * CQ + slot], wh = p.w[h];
            float rsum = 0.f;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt + 16 * n + 4 * g + r;
                    const float pv = (qin && key >= 1 && key <= nn) ? __expf(s[n][r] - m) * il : 0.f;
                    acc[n][r] = __builtin_fmaf(wh, pv, acc[n][r]);
                    rsum += pv;
                    s[n][r] = pv;
                }
            rsum += __shfl_xor(rsum, 16, 64);
            rsum += __shfl_xor(rsum, 32, 64);
            if (g == 0) s_rs[h * CQ + slot] += rsum;
            // column sums over the wave's 16 queries (lanes li = 0 .. 15 of each key group)
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = s[n][r];
                    v += __shfl_xor(v, 1, 64);
                    v += __shfl_xor(v, 2, 64);
                    v += __shfl_xor(v, 4, 64);
                    v += __shfl_xor(v, 8, 64);
                    if (li == 0) s_cs[(h * 4 + wave) * CQ + 16 * n + 4 * g + r] = v;
                }
        }
        __syncthreads();
        // this tile's column partials: the four waves in order
        float *part = p.part + poff * nh + (int64_t)qb * nh * nn;
        for (int i = tid; i < nh * CQ; i += 256) {
            const int h = i / CQ, k = i % CQ, key = kt + k;
            if (key >= 1 && key <= nn) {
                const float *c4 = s_cs + h * 4 * CQ + k;
                part[(int64_t)h * nn + key - 1] = ((c4[0] + c4[CQ]) + c4[2 * CQ]) + c4[3 * CQ];
            }
        }
        if (qin) {
            float *dst = p.A + aoff + (int64_t)(qi - 1) * nn - 1;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt + 16 * n + 4 * g + r;
                    if (key >= 1 && key <= nn) dst[key] = p.accumulate ? dst[key] + acc[n][r] : acc[n][r];
                }
        }
        __syncthreads();                                              // (s_cs is rewritten by the next tile)
    }
    for (int i = tid; i < nh * CQ; i += 256) {
        const int h = i / CQ, q = 1 + qb * CQ + i % CQ;
        if (q <= nn) p.rows[(voff + q - 1) * p.vld + p.c0 + h] = s_rs[i];
    }
}

// vec[i][c0 + h] (+)= sum over the query blocks (in order) of the column partials: thread = (interior position, head) of protein blockIdx.y
__global__ __launch_bounds__(256) void esm_contact_colsum_kernel(const float *__restrict__ part, const int32_t *__restrict__ cu, int heads,
                                                                 float *__restrict__ vec, int64_t vld, int c0, int add) {
    const int b = blockIdx.y;
    const int nn = cu[b + 1] - cu[b] - 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (nn <= 0 || idx >= nn * heads) return;
    const int j = idx / heads, h = idx % heads;
    int64_t aoff, poff;
    contact_offsets(cu, b, aoff, poff);
    const int nqb = (nn + CQ - 1) / CQ;
    const float *src = part + poff * heads + (int64_t)h * nn + j;
    float v = 0.f;
    for (int q = 0; q < nqb; ++q) v += src[(int64_t)q * heads * nn];
    float *dst = vec + (cu[b] - 2 * (int64_t)b + j) * vld + c0 + h;
    *dst = add ? *dst + v : v;
}

// sw[b][c] = w_c / s_c, s_c = sum_i a_c[i] of protein b (fp64 sum in row order)
__global__ __launch_bounds__(256) void esm_contact_scale_kernel(const float *__restrict__ vec, const int32_t *__restrict__ cu, int C,
                                                                const float *__restrict__ w, float *__restrict__ sw) {
    const int b = blockIdx.x;
    const int nn = cu[b + 1] - cu[b] - 2;
    const float *v = vec + (cu[b] - 2 * (int64_t)b) * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int i = 0; i < nn; ++i) s += v[(int64_t)i * C + c];
        sw[(int64_t)b * C + c] = s > 0.0 ? w[c] / (float)s : 0.f;
    }
}

// out = sigmoid(bias + A + A^T - sum_c sw_c a_c a_c^T) for one 64 x 64 tile of protein blockIdx.z; the rank-C product in exact
// fp32 FMAs over 32-channel slices staged in LDS (thread: rows ty + 16 r, columns tx + 16 c)
__global__ __launch_bounds__(256) void esm_contact_finish_kernel(const float *__restrict__ A, const float *__restrict__ vec,
                                                                 const float *__restrict__ sw, const int32_t *__restrict__ cu, int C,
                                                                 const float *__restrict__ bias, float *__restrict__ out) {
    constexpr int KC = 32;
    __shared__ float sU[KC][CQ + 1], sV[KC][CQ + 1];
    const int b = blockIdx.z, nn = cu[b + 1] - cu[b] - 2;
    const int i0 = blockIdx.y * CQ, j0 = blockIdx.x * CQ;
    if (i0 >= nn || j0 >= nn) return;                                 // (uniform)
    int64_t aoff, poff;
    contact_offsets(cu, b, aoff, poff);
    const float *v = vec + (cu[b] - 2 * (int64_t)b) * C;
    const float *swb = sw + (int64_t)b * C;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int k0 = 0; k0 < C; k0 += KC) {
        for (int e = tid; e < KC * CQ; e += 256) {
            const int k = e % KC, r = e / KC, c = k0 + k;
            const int i = i0 + r, j = j0 + r;
            sU[k][r] = (i < nn && c < C) ? v[(int64_t)i * C + c] * swb[c] : 0.f;
            sV[k][r] = (j < nn && c < C) ? v[(int64_t)j * C + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < KC; ++k) {
            float u[4], w4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) u[r] = sU[k][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) w4[c] = sV[k][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_fmaf(u[r], w4[c], acc[r][c]);
        }
        __syncthreads();
    }
    const float bs = bias[0];
    const float *Ab = A + aoff;
    float *ob = out + aoff;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty + 16 * r;
        if (i >= nn) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx + 16 * c;
            if (j >= nn) continue;
            const float x = ((bs + Ab[(int64_t)i * nn + j]) + Ab[(int64_t)j * nn + i]) - acc[r][c];
            ob[(int64_t)i * nn + j] = 1.0f / (1.0f + expf(-x));
        }
    }
}

size_t contact_accum_lds(int heads) { return (size_t)heads * CQ * 7 * sizeof(float); }

template <int HD>
static hipError_t launch_accum_hd(const ContactParams &p, int nqb, hipStream_t s) {
    const size_t lds = contact_accum_lds(p.heads);
    hipError_t e = ensure_dyn_lds(reinterpret_cast<const void *>(&esm_contact_accum_kernel<HD>), lds);
    if (e != hipSuccess) return e;
    OPUS_LAUNCH(KC_CONTACT, (esm_contact_accum_kernel<HD>), dim3(nqb, p.B), dim3(256), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_esm_contact_accum(const ContactParams &p, int head_dim, int max_n, hipStream_t s) {
    const int nqb = (max_n + CQ - 1) / CQ;
    if (nqb <= 0 || p.B <= 0) return hipSuccess;
    if (p.heads < 1 || contact_accum_lds(p.heads) > 160 * 1024 || (p.ld & 7)) return hipErrorInvalidValue;
    switch (head_dim) {
        case 16: return launch_accum_hd<16>(p, nqb, s);
        case 32: return launch_accum_hd<32>(p, nqb, s);
        case 64: return launch_accum_hd<64>(p, nqb, s);
        case 128: return launch_accum_hd<128>(p, nqb, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_esm_contact_colsum(const float *part, const int32_t *cu, int B, int heads, int max_n, float *vec, int64_t vld, int c0,
                                     int add, hipStream_t s) {
    if (max_n <= 0 || B <= 0) return hipSuccess;
    OPUS_LAUNCH(KC_CONTACT, esm_contact_colsum_kernel, dim3(cdiv((int64_t)max_n * heads, 256), B), dim3(256), 0, s, part, cu, heads, vec,
                vld, c0, add);
    return hipGetLastError();
}

hipError_t launch_esm_contact_scale(const float *vec, const int32_t *cu, int B, int C, const float *w, float *sw, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    OPUS_LAUNCH(KC_CONTACT, esm_contact_scale_kernel, dim3(B), dim3(256), 0, s, vec, cu, C, w, sw);
    return hipGetLastError();
}

hipError_t launch_esm_contact_finish(const float *A, const float *vec, const float *sw, const int32_t *cu, int B, int C, int max_n,
                                     const float *bias, float *out, hipStream_t s) {
    if (max_n <= 0 || B <= 0) return hipSuccess;
    const int nt = cdiv(max_n, CQ);
    OPUS_LAUNCH(KC_CONTACT, esm_contact_finish_kernel, dim3(nt, nt, B), dim3(256), 0, s, A, vec, sw, cu, C, bias, out);
    return hipGetLastError();
}

}  // namespace opus
