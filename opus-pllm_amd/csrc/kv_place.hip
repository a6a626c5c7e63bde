// Bandwidth kernels of detached prefixes: a prefix's K / V leaves the context's cache as a snapshot (kv_export_kernel), comes back
// into the decode rows that continue it (kv_place_kernel), and the suffix rows' own K / V is appended behind it (kv_append_kernel).
// kv_export_rows_kernel is kv_place_kernel's inverse for the ragged cache a decode loop leaves behind: per row its own window of
// slots, right-aligned in the snapshot, zeros in front.
//
// K is stored rotated by slot - kstart, so a row's visible slots can be moved to other slots unchanged as long as the row's kstart
// moves with them: kv_place_kernel copies bits and computes nothing.
//
// Snapshot layout: [layers][rows][nkv][T][hd] in the operand dtype, slot 0 first - per (layer, row, kv head) one contiguous block
// of T hd halfs, as the cache holds it (there the block is the head of a cache_sh-long row).  All copies move 16 bytes per lane
// (hd is a multiple of 8 - the launchers check it - and every block starts 16-byte aligned).  All four launch through
// OPUS_LAUNCH, so that in timing mode each record carries the dispatch's own timestamps.
#include "common.h"

namespace opus {

namespace {

constexpr int CHUNK_BLOCKS = 16;   // workgroups that share one contiguous block (grid-stride over its 16-byte pieces)

// grid (layers R nkv, <= CHUNK_BLOCKS, 2): z = 0 copies K, 1 copies V
__global__ __launch_bounds__(256) void kv_export_kernel(const half_t *__restrict__ kc, const half_t *__restrict__ vc, int64_t cache_sl,
                                                        int64_t cache_sb, int64_t cache_sh, int R, int nkv, int64_t blk8,
                                                        half_t *__restrict__ snap_k, half_t *__restrict__ snap_v) {
    const int id = blockIdx.x, h = id % nkv, r = (id / nkv) % R, l = id / (nkv * R);
    const half_t *src = (blockIdx.z ? vc : kc) + l * cache_sl + r * cache_sb + h * cache_sh;
    half_t *dst = (blockIdx.z ? snap_v : snap_k) + (int64_t)id * blk8 * 8;
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < blk8; i += (int64_t)gridDim.y * 256)
        reinterpret_cast<h8 *>(dst)[i] = reinterpret_cast<const h8 *>(src)[i];
}

// grid (layers R nkv, <= CHUNK_BLOCKS, 2): a workgroup takes (layer, row, kv head) and a share of the snapshot block's Tp x hd halfs:
// zeros below the row's first visible slot, behind them the row's window of the cache, bits unchanged
__global__ __launch_bounds__(256) void kv_export_rows_kernel(KvExportRowsParams p) {
    const int id = blockIdx.x, h = id % p.nkv, r = (id / p.nkv) % p.R, l = id / (p.nkv * p.R);
    const int c8 = p.hd >> 3;
    const int64_t blk8 = (int64_t)p.Tp * c8, pad8 = (int64_t)p.nks[r] * c8;
    const half_t *src = (blockIdx.z ? p.vc : p.kc) + l * p.cache_sl + r * p.cache_sb + h * p.cache_sh + (int64_t)p.kstart[r] * p.hd;
    half_t *dst = (blockIdx.z ? p.snap_v : p.snap_k) + (int64_t)id * blk8 * 8;
    const h8 zero = {};
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < blk8; i += (int64_t)gridDim.y * 256)
        reinterpret_cast<h8 *>(dst)[i] = i < pad8 ? zero : reinterpret_cast<const h8 *>(src)[i - pad8];
}

// grid (layers P nkv, <= CHUNK_BLOCKS, 2): a workgroup takes (layer, prefix row, kv head) and a share of the row's Lp x hd block
__global__ __launch_bounds__(256) void kv_place_kernel(KvPlaceParams p) {
    const int id = blockIdx.x, h = id % p.nkv, pr = (id / p.nkv) % p.P, l = id / (p.nkv * p.P);
    const int lo = p.off[pr], hi = p.off[pr + 1];
    if (lo == hi) return;                                          // (no decode row continues this prefix row)
    const int kbeg = p.kstart[pr];
    const int64_t blk8 = (int64_t)(p.Tp - kbeg) * (p.hd >> 3);
    const half_t *src = (blockIdx.z ? p.snap_v : p.snap_k) + ((int64_t)id * p.Tp + kbeg) * p.hd;
    half_t *cache = (blockIdx.z ? p.vc : p.kc) + l * p.cache_sl + h * p.cache_sh;
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < blk8; i += (int64_t)gridDim.y * 256) {
        const h8 v = reinterpret_cast<const h8 *>(src)[i];
        for (int k = lo; k < hi; ++k) {
            const int r = p.list[k];
            reinterpret_cast<h8 *>(cache + r * p.cache_sb + (int64_t)p.new_kstart[r] * p.hd)[i] = v;
        }
    }
}

// one thread per (row, position, kv head, 16-byte piece); K and V
__global__ __launch_bounds__(256) void kv_append_kernel(const half_t *__restrict__ qkv, const int32_t *__restrict__ lens, int n, int nh,
                                                        int nkv, int hd, int Tp, half_t *__restrict__ kc, half_t *__restrict__ vc,
                                                        int64_t cache_sb, int64_t cache_sh, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = hd >> 3, c = (int)(i % c8);
    int64_t q = i / c8;
    const int h = (int)(q % nkv); q /= nkv;
    const int t = (int)(q % n), r = (int)(q / n);
    const int len = lens[r];
    if (t >= len) return;                                          // (right padding)
    const half_t *ks = qkv + (q * (nh + 2 * nkv) + nh + h) * hd + c * 8;
    const int64_t o = r * cache_sb + h * cache_sh + (int64_t)(Tp + n - len + t) * hd + c * 8;
    *reinterpret_cast<h8 *>(kc + o) = *reinterpret_cast<const h8 *>(ks);
    *reinterpret_cast<h8 *>(vc + o) = *reinterpret_cast<const h8 *>(ks + (int64_t)nkv * hd);
}

int chunk_blocks(int64_t blk8) {
    const int64_t nb = (blk8 + 255) / 256;
    return (int)(nb < 1 ? 1 : (nb > CHUNK_BLOCKS ? CHUNK_BLOCKS : nb));
}

}  // namespace

hipError_t launch_kv_export(const half_t *kc, const half_t *vc, int64_t cache_sl, int64_t cache_sb, int64_t cache_sh, int layers, int R,
                            int nkv, int T, int hd, half_t *snap_k, half_t *snap_v, hipStream_t s) {
    if ((hd & 7) || layers < 1 || R < 1 || nkv < 1 || T < 1 || (int64_t)layers * R * nkv >= (1ll << 31)) return hipErrorInvalidValue;
    const int64_t blk8 = (int64_t)T * (hd >> 3);
    OPUS_LAUNCH(KC_OTHER, kv_export_kernel, dim3(layers * R * nkv, chunk_blocks(blk8), 2), dim3(256), 0, s, kc, vc, cache_sl, cache_sb,
                cache_sh, R, nkv, blk8, snap_k, snap_v);
    return hipGetLastError();
}

hipError_t launch_kv_export_rows(const KvExportRowsParams &p, hipStream_t s) {
    if ((p.hd & 7) || p.layers < 1 || p.R < 1 || p.nkv < 1 || p.Tp < 1 || (int64_t)p.layers * p.R * p.nkv >= (1ll << 31))
        return hipErrorInvalidValue;
    OPUS_LAUNCH(KC_OTHER, kv_export_rows_kernel, dim3(p.layers * p.R * p.nkv, chunk_blocks((int64_t)p.Tp * (p.hd >> 3)), 2), dim3(256), 0,
                s, p);
    return hipGetLastError();
}

hipError_t launch_kv_place(const KvPlaceParams &p, hipStream_t s) {
    if ((p.hd & 7) || p.layers < 1 || p.P < 1 || p.nkv < 1 || p.Tp < 1 || (int64_t)p.layers * p.P * p.nkv >= (1ll << 31))
        return hipErrorInvalidValue;
    OPUS_LAUNCH(KC_OTHER, kv_place_kernel, dim3(p.layers * p.P * p.nkv, chunk_blocks((int64_t)p.Tp * (p.hd >> 3)), 2), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_kv_append(const half_t *qkv, const int32_t *lens, int R, int n, int nh, int nkv, int hd, int Tp, half_t *kc, half_t *vc,
                            int64_t cache_sb, int64_t cache_sh, hipStream_t s) {
    if (hd & 7) return hipErrorInvalidValue;
    const int64_t total = (int64_t)R * n * nkv * (hd >> 3);
    OPUS_LAUNCH(KC_OTHER, kv_append_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, qkv, lens, n, nh, nkv, hd, Tp, kc, vc,
                cache_sb, cache_sh, total);
    return hipGetLastError();
}

}  // namespace opus
