"""The GEMM launchers restated, the cells of the GEMM kernels, the case table that fills them and the two input families
(tests/test_gemm_cells_host.py checks all of this on the CPU; tests/gemm_cells_checks.py drives the cases on the GPU).  Needs
torch on the CPU only.  Not product code.

route() is a reading of launch_gemm_ and its sub-launchers (csrc/gemm.hip: launch_skinny_e, launch_wide, launch_mid_t, launch_ring,
launch_tile_e, launch_pp, launch_reduce; csrc/gemm_stream.hip: stream_plan, launch_stream_t) at the default knobs, with no
environment A/B aid set and the context's 64 MiB workspace, written from their rules and not generated from them.  It returns the
report the launchers give through GemmParams::plan (opus_debug_gemm_plan).  Where the two disagree the launcher is the truth about
routing and this file is what gets corrected.

A cell is (kernel instantiation as reported) x (epilogue, output mode) x (how the k-parts become the output).  The (epilogue,
output mode) pairs are the ones the product path issues: the plain epilogue in fp16, in fp32 onto the residual aliased to C, and in
fp32 without a residual (lm_head); GELU and the gate / up pair in fp16.  With the RMSNorm fused (fp32 activations, skinny and mid
kernels only): plain fp16, plain fp32 (lm_head), gate / up fp16.  Tuples of the older parity tables that lie outside these pairs
(GELU with fp32 + residual on the big tiled GEMM) stay in the table; their cells are listed in EXTRA_CELLS.
"""
from __future__ import annotations

from collections import namedtuple

import torch

WS_BYTES = 64 << 20
SKINNY, MID, WIDE, RING, PP, TILE, STREAM = "gemm_skinny", "gemm_mid", "gemm_wide", "gemm_ring", "gemm_pp", "gemm_tile", "gemm_stream"
PLAIN, GELU, SILU = 0, 1, 2
F16, F32R, F32 = "f16", "f32+res", "f32"           # fp16 without residual / fp32 with the residual aliased to C / fp32 without residual
NONE, REDUCE, REDUCE4, IN_LAUNCH, PP_PAIR, PP_REDUCE, SLABS = range(7)
COMBINE_NAMES = ("one k-part", "splitk_reduce", "splitk_reduce4", "in launch", "pp pair", "pp_tail_reduce", "slabs")
SKINNY_MAX_M, MID_MAX_M = 4, 64

Plan = namedtuple("Plan", "klass mt tn ns alds P ks combine")


def cdiv(a, b):
    return -(-a // b)


def _shrink(ks, bytes_of):
    while ks > 1 and bytes_of(ks) > WS_BYTES:
        ks -= 1
    return max(ks, 1)


def _reduce_kind(N, epi):
    # launch_reduce: the 4-wide plain reduce wants whole 256-column blocks (ldc = ldr = N there, so the strides follow)
    return REDUCE4 if epi == PLAIN and N % 256 == 0 else REDUCE


def stream_plan(M, N, K, slab_only, a_tiled):
    """(P, ks) of gemm_stream_kernel or None: P panels per workgroup x ks k-parts on 192 .. 256 workgroups."""
    if N % 16 or K % 64 or not 1 <= M <= 64:
        return None
    npanels, chunks, best, pick = N // 16, K // 64, 0, None
    for P, ks in ((1, 1), (3, 2), (3, 4), (4, 4), (5, 4)):
        if npanels % P or (P == 3 and not slab_only) or (P >= 4 and (slab_only or not a_tiled)) or (P == 5 and M > 48):
            continue
        nt = 1024 if P == 1 else 512
        wgs = npanels // P * ks
        if chunks // ks < nt // 64 or not 192 <= wgs <= 256:
            continue
        if (ks > 1 and ks * M * N * 4 > WS_BYTES) or 2 * M * K // ks > (600 if a_tiled else 280) * 1024:
            continue
        if wgs > best:                     # ties: the earlier candidate
            best, pick = wgs, (P, ks)
    return pick


def _ring(M, N, K, epi, TM, TN, NS, allow_split):
    tiles = cdiv(M, 32 * TM) * cdiv(N, 64 * TN)
    ks = 1
    if allow_split and tiles < 200:
        floor = 256 // tiles
        ks = floor if (floor >= 2 or K <= 2048) else cdiv(256, tiles)
        ks = min(max(ks, 1), 16, (K // 32) // 8)
        ks = _shrink(ks, lambda k: k * M * N * 4)
    return Plan(RING, TM, TN, NS, 0, 0, ks, NONE if ks == 1 else _reduce_kind(N, epi))


def _pp(M, N, K, epi, mode):
    T, KT = cdiv(M, 256) * cdiv(N, 256), K // 64
    R, split = T % 256, 1
    if T > 256 and 0 < R <= 128:
        sp = min(256 // R, 8, KT // 4)
        sp = _shrink(sp, lambda k: (R * k) << 18) if sp > 1 else sp
        if sp > 1 and (1.5 * KT + 12.0) * (1.0 - 1.0 / sp) > (22.0 if sp == 2 else 30.0):
            split = sp
    nout = N // 2 if epi == SILU else N
    pair = split == 2 and (mode == F16 or (mode == F32R and epi == PLAIN)) and nout % 8 == 0 and N % 256 == 0
    return Plan(PP, 0, 0, 0, 0, 0, split, NONE if split == 1 else PP_PAIR if pair else PP_REDUCE)


def route(M, N, K, epi, mode, norm=False, a_tiled=False, slab_only=False):
    """The launchers' report for C[M, Nout] = epi(A[M, K] W[N, K]^T + bias) (+ residual), or None where launch_gemm_ refuses.
    slab_only is opus_debug_gemm_slabs (which also forces a narrow output onto gemm_wide_kernel when the stream kernel does not
    take it)."""
    if M < 1 or N < 1 or K < 64 or K % 64 or (epi == SILU and N % 32) or (norm and (epi == GELU or M > MID_MAX_M)):
        return None
    chunks = K // 64
    if M <= SKINNY_MAX_M:
        if a_tiled:
            return None
        return Plan(SKINNY, 1, 0, 0, 1 if M * K * 2 <= 64 * 1024 else 0, 0, 1, NONE)
    mid = M <= MID_MAX_M
    if mid and not norm and N < 16384 and epi in (PLAIN, GELU) and (a_tiled or (M - 1) * K + K < 1 << 29):
        pl = stream_plan(M, N, K, slab_only, a_tiled)
        if pl:
            P, ks = pl
            return Plan(STREAM, cdiv(M, 16), 0, 0, 0, P, ks, NONE if ks == 1 else SLABS if slab_only else IN_LAUNCH)
    if a_tiled:
        return None                        # the fragment-ordered activation layout is read by gemm_stream_kernel only
    if not norm and ((mid and (N >= 16384 or slab_only)) or (MID_MAX_M < M <= 96 and N >= 16384)):
        mt = 2 if M <= 32 else 4 if mid else 6
        blocks, ks = cdiv(cdiv(N, 16), 8), 1
        if blocks < 200:
            ks = _shrink(max(min(256 // blocks, 8, chunks // 8), 1), lambda k: k * M * N * 4)
        return Plan(WIDE, mt, 0, 0, 0, 0, ks, NONE if ks == 1 else SLABS if slab_only else _reduce_kind(N, epi))
    if mid and not norm and M > 32:
        return _ring(M, N, K, epi, 2, 2, 8, True)
    if mid:
        blocks, ks = cdiv(cdiv(N, 16), 4), 1
        if blocks < 384:
            ks = _shrink(max(min(cdiv(512, blocks), 8, chunks // 4), 1), lambda k: (k * M * N + k * M) * 4)
        return Plan(MID, 2 * cdiv(M, 32), 0, 0, 0, 0, ks, NONE if ks == 1 else _reduce_kind(N, epi))
    if cdiv(M, 256) * cdiv(N, 256) >= 128:
        if M * K * 2 >= 1 << 32 or N * K * 2 >= 1 << 32:          # gemm_pp_kernel's 32-bit byte offsets
            if (mode == F32R or epi == GELU) and K <= 4096:
                return _ring(M, N, K, epi, 4, 2, 4, False)
            return _ring(M, N, K, epi, 8, 4, 4, False)
        return _pp(M, N, K, epi, mode)
    if M > 128:
        return _ring(M, N, K, epi, 4, 2, 4, True)
    ntile, ks = cdiv(M, 128) * cdiv(N, 128), 1
    if ntile < 160:
        ks = _shrink(max(min(320 // ntile, 8, chunks // 4), 1), lambda k: k * M * N * 4)
    return Plan(TILE, 0, 0, 0, 0, 0, ks, NONE if ks == 1 else _reduce_kind(N, epi))


# ------------------------------------------------------------------------------------------------ cells
PAIRS = ((PLAIN, F16), (PLAIN, F32R), (PLAIN, F32), (GELU, F16), (SILU, F16))      # (epilogue, output mode) on fp16 activations
NORM_PAIRS = ((PLAIN, F16), (PLAIN, F32), (SILU, F16))                             # with the RMSNorm fused (fp32 activations)
Cell = namedtuple("Cell", "klass mt tn ns alds P norm epi mode combine")


def _kinds(epi):
    """k-parts summed by a reduce launch: the 4-wide plain reduce when N % 256 == 0, the generic one otherwise / with an activation"""
    return (NONE, REDUCE, REDUCE4) if epi == PLAIN else (NONE, REDUCE)


def _cells():
    out = []
    for alds in (1, 0):                                        # skinny: <= 4 rows; !ALDS from M K 2 > 64 KiB (K > 8192 at 4 rows)
        out += [Cell(SKINNY, 1, 0, 0, alds, 0, n, e, m, NONE) for n in (False, True) for e, m in (NORM_PAIRS if n else PAIRS)]
    # mid: 5 .. 32 rows on fp16 activations, 5 .. 64 rows with the norm fused (gemm_mid_kernel<6 / 8>: beyond MID_MAX_M, never launched)
    for mt, norms in ((2, (False, True)), (4, (True,))):
        out += [Cell(MID, mt, 0, 0, 0, 0, n, e, m, k) for n in norms for e, m in (NORM_PAIRS if n else PAIRS) for k in _kinds(e)]
    # wide: N >= 16384; its k-parts need <= 128 column blocks, i.e. N == 16384, so the plain epilogue only meets the 4-wide reduce
    for mt in (2, 4, 6):
        out += [Cell(WIDE, mt, 0, 0, 0, 0, False, e, m, k) for e, m in PAIRS for k in (NONE, REDUCE4 if e == PLAIN else REDUCE)]
    for inst in ((RING, 2, 2, 8), (RING, 4, 2, 4), (TILE, 0, 0, 0)):
        out += [Cell(*inst, 0, 0, False, e, m, k) for e, m in PAIRS for k in _kinds(e)]
    # stream: plain / GELU; one panel per workgroup and the whole K, or 4 / 5 panels x 4 k-parts (fragment-ordered activations only)
    for P, mts, k in ((1, (1, 2, 3, 4), NONE), (4, (1, 2, 3, 4), IN_LAUNCH), (5, (1, 2, 3), IN_LAUNCH)):
        out += [Cell(STREAM, mt, 0, 0, 0, P, False, e, m, k) for mt in mts for e, m in PAIRS if e != SILU]
    # the big tiled GEMM: no tail split, tail tiles through pp_tail_reduce_kernel, two-part tail tiles exchanged inside the launch
    # (the pair hand-off carries fp16 without a residual, and fp32 + residual in the plain epilogue)
    out += [Cell(PP, 0, 0, 0, 0, 0, False, e, m, k) for e, m in PAIRS for k in (NONE, PP_REDUCE)]
    out += [Cell(PP, 0, 0, 0, 0, 0, False, e, m, PP_PAIR) for e, m in PAIRS if m != F32]
    return out


CELLS = _cells()
# raw slabs left for the consumer (opus_debug_gemm_slabs: the QKV projection of the batched decode step)
SLAB_CELLS = [Cell(STREAM, 2, 0, 0, 0, 3, False, PLAIN, F16, SLABS), Cell(WIDE, 2, 0, 0, 0, 0, False, PLAIN, F16, SLABS),
              Cell(WIDE, 4, 0, 0, 0, 0, False, PLAIN, F16, SLABS)]
# cells of older table tuples outside the product path's (epilogue, output mode) pairs
EXTRA_CELLS = [Cell(PP, 0, 0, 0, 0, 0, False, GELU, F32R, PP_REDUCE)]
# Not covered, by choice: reachable only through an environment A/B aid or a run-time knob.
NOT_COVERED = (
    "OPUS_SKINNY_MAX_M > 4: gemm_skinny_kernel at 5 .. 16 rows (<1, .., ALDS> up to 16 rows, <1 / 2 / 4, .., !ALDS> beyond)",
    "OPUS_SKINNY_W: another number of waves per skinny workgroup",
    "OPUS_NO_MID_GEMM, OPUS_MID_V1: gemm_mid_kernel<6 / 8> and the mid kernel on shapes the stream / wide / ring kernels take",
    "OPUS_NARROW_WIDE: gemm_wide_kernel with k-parts on narrow outputs (opus_debug_gemm_slabs reaches it, SLAB_CELLS)",
    "OPUS_NO_STREAM / knob no_stream: stream shapes on the mid / ring kernels (same instantiations as the cells above)",
    "OPUS_NO_COMBINE / knob misc4: gemm_stream_kernel's k-parts through splitk_reduce",
    "knob misc6: two-part tail tiles of gemm_pp_kernel through pp_tail_reduce_kernel in the pair modes",
    "OPUS_NO_PP_TAIL, OPUS_NO_BIG_GEMM, OPUS_PP_MIN_TILES, OPUS_NO_SMALL_RING, OPUS_NO_KROT, OPUS_NO_ROPE_FUSION",
    "OPUS_NO_PP: gemm_ring_kernel<8,4,4> / unsplit <4,2,4> - with default knobs only behind the 4 GiB guard, which keeps its own "
    "test (tests/test_gpu_parity.py::test_gemm_operand_of_4_gib_takes_64_bit_addressing)",
)

# ------------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "M N K epi mode plan norm a_tiled slab")


def C(M, N, K, epi, mode, plan, norm=False, a_tiled=False, slab=False):
    return Case(M, N, K, epi, mode, plan, norm, a_tiled, slab)


# every tuple of tests/test_gpu_parity.py::test_gemm_kernels, in its order, with the plan each is filed under
OLD_KERNEL_CASES = [
    C(1, 64, 64, PLAIN, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(1, 4096, 4096, PLAIN, F32R, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(3, 160, 320, GELU, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(8, 256, 1280, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 5, REDUCE4)),
    C(16, 512, 128, SILU, F16, Plan(MID, 2, 0, 0, 0, 0, 1, NONE)),
    C(17, 96, 192, PLAIN, F32R, Plan(MID, 2, 0, 0, 0, 0, 1, NONE)),
    C(33, 64, 256, GELU, F16, Plan(RING, 2, 2, 8, 0, 0, 1, NONE)),
    C(64, 1024, 512, SILU, F16, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE)),
    C(48, 4096, 4096, PLAIN, F32R, Plan(RING, 2, 2, 8, 0, 0, 8, REDUCE4)),
    C(96, 6144, 4096, PLAIN, F16, Plan(TILE, 0, 0, 0, 0, 0, 6, REDUCE4)),
    C(128, 1056, 1280, GELU, F16, Plan(TILE, 0, 0, 0, 0, 0, 5, REDUCE)),
    C(70, 4096, 14336, PLAIN, F32R, Plan(TILE, 0, 0, 0, 0, 0, 8, REDUCE4)),
    C(65, 128, 64, PLAIN, F16, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(130, 384, 320, GELU, F16, Plan(RING, 4, 2, 4, 0, 0, 1, NONE)),
    C(257, 200, 128, PLAIN, F32R, Plan(RING, 4, 2, 4, 0, 0, 1, NONE)),
    C(300, 512, 1280, SILU, F16, Plan(RING, 4, 2, 4, 0, 0, 5, REDUCE)),
    C(514, 3840, 1280, PLAIN, F16, Plan(RING, 4, 2, 4, 0, 0, 1, NONE)),
    C(1, 32768, 5120, GELU, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(24, 16384, 1024, PLAIN, F16, Plan(WIDE, 2, 0, 0, 0, 0, 2, REDUCE4)),
    C(32, 16416, 4096, SILU, F16, Plan(WIDE, 2, 0, 0, 0, 0, 1, NONE)),
    C(64, 20480, 1088, GELU, F16, Plan(WIDE, 4, 0, 0, 0, 0, 1, NONE)),
    C(90, 16384, 576, SILU, F16, Plan(WIDE, 6, 0, 0, 0, 0, 1, NONE)),
    C(4100, 3000, 320, GELU, F16, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(3000, 4100, 64, PLAIN, F32R, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(2600, 5120, 128, SILU, F16, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(3900, 3328, 640, PLAIN, F16, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(1300, 11100, 1280, PLAIN, F16, Plan(PP, 0, 0, 0, 0, 0, 5, PP_REDUCE)),
    C(1280, 13312, 1024, SILU, F16, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(2304, 7424, 1280, GELU, F16, Plan(PP, 0, 0, 0, 0, 0, 5, PP_REDUCE)),
    C(4608, 4608, 512, PLAIN, F32R, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(6144, 4096, 4096, PLAIN, F32R, Plan(PP, 0, 0, 0, 0, 0, 2, PP_PAIR)),
    C(3072, 8192, 3072, GELU, F16, Plan(PP, 0, 0, 0, 0, 0, 2, PP_PAIR)),
    C(3072, 16384, 3072, SILU, F16, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(16000, 2560, 2560, GELU, F32R, Plan(PP, 0, 0, 0, 0, 0, 2, PP_REDUCE)),
]
# every tuple of tests/test_gpu_parity.py::test_gemm_fused_rmsnorm
OLD_NORM_CASES = [
    C(1, 256, 4096, PLAIN, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE), norm=True),
    C(5, 512, 1024, SILU, F16, Plan(MID, 2, 0, 0, 0, 0, 4, REDUCE), norm=True),
    C(16, 96, 320, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 1, NONE), norm=True),
    C(17, 6144, 4096, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 6, REDUCE4), norm=True),
    C(40, 640, 1280, SILU, F16, Plan(MID, 4, 0, 0, 0, 0, 5, REDUCE), norm=True),
    C(64, 4096, 4096, PLAIN, F16, Plan(MID, 4, 0, 0, 0, 0, 8, REDUCE4), norm=True),
    C(64, 28672, 4096, SILU, F16, Plan(MID, 4, 0, 0, 0, 0, 1, NONE), norm=True),
    C(50, 208, 192, PLAIN, F16, Plan(MID, 4, 0, 0, 0, 0, 1, NONE), norm=True),
    C(33, 2048, 512, SILU, F16, Plan(MID, 4, 0, 0, 0, 0, 2, REDUCE), norm=True),
    C(60, 4096, 14336, PLAIN, F16, Plan(MID, 4, 0, 0, 0, 0, 8, REDUCE4), norm=True),
]
# the smallest shape found for every cell (rows off the row tile, columns off 16 wherever the kernel admits it; three 64-k chunks at
# the least), then shapes of the product path and the row counts around MID_MAX_M
NEW_CASES = [
    C(5, 200, 192, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 200, 512, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE)),
    C(5, 1280, 512, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE4)),
    C(5, 200, 192, PLAIN, F32, Plan(MID, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 200, 512, PLAIN, F32, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE)),
    C(5, 1280, 512, PLAIN, F32, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE4)),
    C(5, 200, 192, PLAIN, F32R, Plan(MID, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 200, 512, PLAIN, F32R, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE)),
    C(5, 1280, 512, PLAIN, F32R, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE4)),
    C(5, 200, 192, GELU, F16, Plan(MID, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 200, 512, GELU, F16, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE)),
    C(5, 96, 192, SILU, F16, Plan(MID, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 96, 512, SILU, F16, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE)),
    C(5, 200, 192, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 1, NONE), norm=True),
    C(5, 200, 512, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE), norm=True),
    C(5, 1280, 512, PLAIN, F16, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE4), norm=True),
    C(5, 200, 192, PLAIN, F32, Plan(MID, 2, 0, 0, 0, 0, 1, NONE), norm=True),
    C(5, 200, 512, PLAIN, F32, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE), norm=True),
    C(5, 1280, 512, PLAIN, F32, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE4), norm=True),
    C(5, 96, 192, SILU, F16, Plan(MID, 2, 0, 0, 0, 0, 1, NONE), norm=True),
    C(5, 96, 512, SILU, F16, Plan(MID, 2, 0, 0, 0, 0, 2, REDUCE), norm=True),
    C(37, 200, 192, PLAIN, F16, Plan(MID, 4, 0, 0, 0, 0, 1, NONE), norm=True),
    C(37, 200, 512, PLAIN, F16, Plan(MID, 4, 0, 0, 0, 0, 2, REDUCE), norm=True),
    C(37, 1280, 512, PLAIN, F16, Plan(MID, 4, 0, 0, 0, 0, 2, REDUCE4), norm=True),
    C(37, 200, 192, PLAIN, F32, Plan(MID, 4, 0, 0, 0, 0, 1, NONE), norm=True),
    C(37, 200, 512, PLAIN, F32, Plan(MID, 4, 0, 0, 0, 0, 2, REDUCE), norm=True),
    C(37, 1280, 512, PLAIN, F32, Plan(MID, 4, 0, 0, 0, 0, 2, REDUCE4), norm=True),
    C(37, 96, 192, SILU, F16, Plan(MID, 4, 0, 0, 0, 0, 1, NONE), norm=True),
    C(37, 96, 512, SILU, F16, Plan(MID, 4, 0, 0, 0, 0, 2, REDUCE), norm=True),
    C(37, 200, 192, PLAIN, F16, Plan(RING, 2, 2, 8, 0, 0, 1, NONE)),
    C(37, 200, 512, PLAIN, F16, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE)),
    C(37, 1280, 512, PLAIN, F16, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE4)),
    C(37, 200, 192, PLAIN, F32, Plan(RING, 2, 2, 8, 0, 0, 1, NONE)),
    C(37, 200, 512, PLAIN, F32, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE)),
    C(37, 1280, 512, PLAIN, F32, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE4)),
    C(37, 200, 192, PLAIN, F32R, Plan(RING, 2, 2, 8, 0, 0, 1, NONE)),
    C(37, 200, 512, PLAIN, F32R, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE)),
    C(37, 1280, 512, PLAIN, F32R, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE4)),
    C(37, 200, 192, GELU, F16, Plan(RING, 2, 2, 8, 0, 0, 1, NONE)),
    C(37, 200, 512, GELU, F16, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE)),
    C(37, 96, 192, SILU, F16, Plan(RING, 2, 2, 8, 0, 0, 1, NONE)),
    C(37, 96, 512, SILU, F16, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE)),
    C(130, 200, 192, PLAIN, F16, Plan(RING, 4, 2, 4, 0, 0, 1, NONE)),
    C(130, 200, 512, PLAIN, F16, Plan(RING, 4, 2, 4, 0, 0, 2, REDUCE)),
    C(130, 1280, 512, PLAIN, F16, Plan(RING, 4, 2, 4, 0, 0, 2, REDUCE4)),
    C(130, 200, 192, PLAIN, F32, Plan(RING, 4, 2, 4, 0, 0, 1, NONE)),
    C(130, 200, 512, PLAIN, F32, Plan(RING, 4, 2, 4, 0, 0, 2, REDUCE)),
    C(130, 1280, 512, PLAIN, F32, Plan(RING, 4, 2, 4, 0, 0, 2, REDUCE4)),
    C(130, 200, 192, PLAIN, F32R, Plan(RING, 4, 2, 4, 0, 0, 1, NONE)),
    C(130, 200, 512, PLAIN, F32R, Plan(RING, 4, 2, 4, 0, 0, 2, REDUCE)),
    C(130, 1280, 512, PLAIN, F32R, Plan(RING, 4, 2, 4, 0, 0, 2, REDUCE4)),
    C(130, 200, 192, GELU, F16, Plan(RING, 4, 2, 4, 0, 0, 1, NONE)),
    C(130, 200, 512, GELU, F16, Plan(RING, 4, 2, 4, 0, 0, 2, REDUCE)),
    C(130, 96, 192, SILU, F16, Plan(RING, 4, 2, 4, 0, 0, 1, NONE)),
    C(130, 96, 512, SILU, F16, Plan(RING, 4, 2, 4, 0, 0, 2, REDUCE)),
    C(4, 200, 8256, PLAIN, F16, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE)),
    C(4, 200, 8256, PLAIN, F32, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE)),
    C(4, 200, 8256, PLAIN, F32R, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE)),
    C(4, 200, 8256, GELU, F16, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE)),
    C(4, 96, 8256, SILU, F16, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE)),
    C(1, 200, 192, PLAIN, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(1, 200, 192, PLAIN, F32, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(1, 200, 192, PLAIN, F32R, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(1, 200, 192, GELU, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(1, 96, 192, SILU, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE)),
    C(4, 200, 8256, PLAIN, F16, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE), norm=True),
    C(4, 200, 8256, PLAIN, F32, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE), norm=True),
    C(4, 96, 8256, SILU, F16, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE), norm=True),
    C(1, 200, 192, PLAIN, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE), norm=True),
    C(1, 200, 192, PLAIN, F32, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE), norm=True),
    C(1, 96, 192, SILU, F16, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE), norm=True),
    C(5, 3072, 1024, PLAIN, F16, Plan(STREAM, 1, 0, 0, 0, 1, 1, NONE)),
    C(5, 3072, 1024, PLAIN, F32, Plan(STREAM, 1, 0, 0, 0, 1, 1, NONE)),
    C(5, 3072, 1024, PLAIN, F32R, Plan(STREAM, 1, 0, 0, 0, 1, 1, NONE)),
    C(5, 3072, 1024, GELU, F16, Plan(STREAM, 1, 0, 0, 0, 1, 1, NONE)),
    C(15, 3072, 20544, PLAIN, F16, Plan(STREAM, 1, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(15, 3072, 20544, PLAIN, F32, Plan(STREAM, 1, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(15, 3072, 20544, PLAIN, F32R, Plan(STREAM, 1, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(15, 3072, 20544, GELU, F16, Plan(STREAM, 1, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(5, 4160, 2048, PLAIN, F16, Plan(STREAM, 1, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(5, 4160, 2048, PLAIN, F32, Plan(STREAM, 1, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(5, 4160, 2048, PLAIN, F32R, Plan(STREAM, 1, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(5, 4160, 2048, GELU, F16, Plan(STREAM, 1, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(20, 3072, 1024, PLAIN, F16, Plan(STREAM, 2, 0, 0, 0, 1, 1, NONE)),
    C(20, 3072, 1024, PLAIN, F32, Plan(STREAM, 2, 0, 0, 0, 1, 1, NONE)),
    C(20, 3072, 1024, PLAIN, F32R, Plan(STREAM, 2, 0, 0, 0, 1, 1, NONE)),
    C(20, 3072, 1024, GELU, F16, Plan(STREAM, 2, 0, 0, 0, 1, 1, NONE)),
    C(27, 3072, 14336, PLAIN, F16, Plan(STREAM, 2, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(27, 3072, 14336, PLAIN, F32, Plan(STREAM, 2, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(27, 3072, 14336, PLAIN, F32R, Plan(STREAM, 2, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(27, 3072, 14336, GELU, F16, Plan(STREAM, 2, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(20, 4160, 2048, PLAIN, F16, Plan(STREAM, 2, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(20, 4160, 2048, PLAIN, F32, Plan(STREAM, 2, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(20, 4160, 2048, PLAIN, F32R, Plan(STREAM, 2, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(20, 4160, 2048, GELU, F16, Plan(STREAM, 2, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(37, 3072, 1024, PLAIN, F16, Plan(STREAM, 3, 0, 0, 0, 1, 1, NONE)),
    C(37, 3072, 1024, PLAIN, F32, Plan(STREAM, 3, 0, 0, 0, 1, 1, NONE)),
    C(37, 3072, 1024, PLAIN, F32R, Plan(STREAM, 3, 0, 0, 0, 1, 1, NONE)),
    C(37, 3072, 1024, GELU, F16, Plan(STREAM, 3, 0, 0, 0, 1, 1, NONE)),
    C(40, 3072, 8256, PLAIN, F16, Plan(STREAM, 3, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(40, 3072, 8256, PLAIN, F32, Plan(STREAM, 3, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(40, 3072, 8256, PLAIN, F32R, Plan(STREAM, 3, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(40, 3072, 8256, GELU, F16, Plan(STREAM, 3, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(37, 4160, 2048, PLAIN, F16, Plan(STREAM, 3, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(37, 4160, 2048, PLAIN, F32, Plan(STREAM, 3, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(37, 4160, 2048, PLAIN, F32R, Plan(STREAM, 3, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(37, 4160, 2048, GELU, F16, Plan(STREAM, 3, 0, 0, 0, 5, 4, IN_LAUNCH), a_tiled=True),
    C(50, 3072, 1024, PLAIN, F16, Plan(STREAM, 4, 0, 0, 0, 1, 1, NONE)),
    C(50, 3072, 1024, PLAIN, F32, Plan(STREAM, 4, 0, 0, 0, 1, 1, NONE)),
    C(50, 3072, 1024, PLAIN, F32R, Plan(STREAM, 4, 0, 0, 0, 1, 1, NONE)),
    C(50, 3072, 1024, GELU, F16, Plan(STREAM, 4, 0, 0, 0, 1, 1, NONE)),
    C(50, 3072, 8256, PLAIN, F16, Plan(STREAM, 4, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(50, 3072, 8256, PLAIN, F32, Plan(STREAM, 4, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(50, 3072, 8256, PLAIN, F32R, Plan(STREAM, 4, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(50, 3072, 8256, GELU, F16, Plan(STREAM, 4, 0, 0, 0, 4, 4, IN_LAUNCH), a_tiled=True),
    C(70, 200, 192, PLAIN, F16, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(70, 200, 512, PLAIN, F16, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE)),
    C(70, 1280, 512, PLAIN, F16, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE4)),
    C(70, 200, 192, PLAIN, F32, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(70, 200, 512, PLAIN, F32, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE)),
    C(70, 1280, 512, PLAIN, F32, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE4)),
    C(70, 200, 192, PLAIN, F32R, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(70, 200, 512, PLAIN, F32R, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE)),
    C(70, 1280, 512, PLAIN, F32R, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE4)),
    C(70, 200, 192, GELU, F16, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(70, 200, 512, GELU, F16, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE)),
    C(70, 96, 192, SILU, F16, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(70, 96, 512, SILU, F16, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE)),
    C(5, 16392, 192, PLAIN, F16, Plan(WIDE, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 16384, 1024, PLAIN, F16, Plan(WIDE, 2, 0, 0, 0, 0, 2, REDUCE4)),
    C(5, 16392, 192, PLAIN, F32, Plan(WIDE, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 16384, 1024, PLAIN, F32, Plan(WIDE, 2, 0, 0, 0, 0, 2, REDUCE4)),
    C(5, 16392, 192, PLAIN, F32R, Plan(WIDE, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 16384, 1024, PLAIN, F32R, Plan(WIDE, 2, 0, 0, 0, 0, 2, REDUCE4)),
    C(5, 16392, 192, GELU, F16, Plan(WIDE, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 16384, 1024, GELU, F16, Plan(WIDE, 2, 0, 0, 0, 0, 2, REDUCE)),
    C(5, 16384, 192, SILU, F16, Plan(WIDE, 2, 0, 0, 0, 0, 1, NONE)),
    C(5, 16384, 1024, SILU, F16, Plan(WIDE, 2, 0, 0, 0, 0, 2, REDUCE)),
    C(37, 16392, 192, PLAIN, F16, Plan(WIDE, 4, 0, 0, 0, 0, 1, NONE)),
    C(37, 16384, 1024, PLAIN, F16, Plan(WIDE, 4, 0, 0, 0, 0, 2, REDUCE4)),
    C(37, 16392, 192, PLAIN, F32, Plan(WIDE, 4, 0, 0, 0, 0, 1, NONE)),
    C(37, 16384, 1024, PLAIN, F32, Plan(WIDE, 4, 0, 0, 0, 0, 2, REDUCE4)),
    C(37, 16392, 192, PLAIN, F32R, Plan(WIDE, 4, 0, 0, 0, 0, 1, NONE)),
    C(37, 16384, 1024, PLAIN, F32R, Plan(WIDE, 4, 0, 0, 0, 0, 2, REDUCE4)),
    C(37, 16392, 192, GELU, F16, Plan(WIDE, 4, 0, 0, 0, 0, 1, NONE)),
    C(37, 16384, 1024, GELU, F16, Plan(WIDE, 4, 0, 0, 0, 0, 2, REDUCE)),
    C(37, 16384, 192, SILU, F16, Plan(WIDE, 4, 0, 0, 0, 0, 1, NONE)),
    C(37, 16384, 1024, SILU, F16, Plan(WIDE, 4, 0, 0, 0, 0, 2, REDUCE)),
    C(70, 16392, 192, PLAIN, F16, Plan(WIDE, 6, 0, 0, 0, 0, 1, NONE)),
    C(70, 16384, 1024, PLAIN, F16, Plan(WIDE, 6, 0, 0, 0, 0, 2, REDUCE4)),
    C(70, 16392, 192, PLAIN, F32, Plan(WIDE, 6, 0, 0, 0, 0, 1, NONE)),
    C(70, 16384, 1024, PLAIN, F32, Plan(WIDE, 6, 0, 0, 0, 0, 2, REDUCE4)),
    C(70, 16392, 192, PLAIN, F32R, Plan(WIDE, 6, 0, 0, 0, 0, 1, NONE)),
    C(70, 16384, 1024, PLAIN, F32R, Plan(WIDE, 6, 0, 0, 0, 0, 2, REDUCE4)),
    C(70, 16392, 192, GELU, F16, Plan(WIDE, 6, 0, 0, 0, 0, 1, NONE)),
    C(70, 16384, 1024, GELU, F16, Plan(WIDE, 6, 0, 0, 0, 0, 2, REDUCE)),
    C(70, 16384, 192, SILU, F16, Plan(WIDE, 6, 0, 0, 0, 0, 1, NONE)),
    C(70, 16384, 1024, SILU, F16, Plan(WIDE, 6, 0, 0, 0, 0, 2, REDUCE)),
    # shapes of the product path, the rows around MID_MAX_M, the big tiled GEMM's tail forms
    C(4, 4096, 14336, PLAIN, F32R, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE)),
    C(4, 512, 14336, SILU, F16, Plan(SKINNY, 1, 0, 0, 0, 0, 1, NONE), norm=True),
    C(2, 1000, 4096, PLAIN, F32, Plan(SKINNY, 1, 0, 0, 1, 0, 1, NONE), norm=True),
    C(20, 1000, 1024, PLAIN, F32, Plan(MID, 2, 0, 0, 0, 0, 4, REDUCE), norm=True),
    C(12, 6400, 256, GELU, F16, Plan(MID, 2, 0, 0, 0, 0, 1, NONE)),
    C(12, 320, 1280, GELU, F16, Plan(MID, 2, 0, 0, 0, 0, 5, REDUCE)),
    C(16, 4096, 1024, GELU, F16, Plan(STREAM, 1, 0, 0, 0, 1, 1, NONE)),
    C(16, 4096, 1024, PLAIN, F16, Plan(STREAM, 1, 0, 0, 0, 1, 1, NONE)),
    C(20, 32000, 256, PLAIN, F32, Plan(WIDE, 2, 0, 0, 0, 0, 1, NONE)),
    C(40, 32000, 256, PLAIN, F32, Plan(WIDE, 4, 0, 0, 0, 0, 1, NONE)),
    C(80, 16400, 256, PLAIN, F32, Plan(WIDE, 6, 0, 0, 0, 0, 1, NONE)),
    C(20, 16384, 512, GELU, F16, Plan(WIDE, 2, 0, 0, 0, 0, 1, NONE)),
    C(40, 16384, 2048, SILU, F16, Plan(WIDE, 4, 0, 0, 0, 0, 2, REDUCE)),
    C(40, 200, 128, PLAIN, F16, Plan(RING, 2, 2, 8, 0, 0, 1, NONE)),
    C(40, 1280, 2560, GELU, F16, Plan(RING, 2, 2, 8, 0, 0, 10, REDUCE)),
    C(100, 300, 128, GELU, F16, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(100, 320, 128, SILU, F16, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(100, 320, 1024, SILU, F16, Plan(TILE, 0, 0, 0, 0, 0, 4, REDUCE)),
    C(100, 1000, 512, PLAIN, F32, Plan(TILE, 0, 0, 0, 0, 0, 2, REDUCE)),
    C(200, 520, 2048, PLAIN, F32R, Plan(RING, 4, 2, 4, 0, 0, 8, REDUCE)),
    C(3072, 8192, 3072, SILU, F16, Plan(PP, 0, 0, 0, 0, 0, 2, PP_PAIR)),
    C(3000, 3000, 128, PLAIN, F32, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(2900, 3000, 192, PLAIN, F16, Plan(PP, 0, 0, 0, 0, 0, 1, NONE)),
    C(49, 200, 192, PLAIN, F16, Plan(RING, 2, 2, 8, 0, 0, 1, NONE)),
    C(64, 520, 512, PLAIN, F32R, Plan(RING, 2, 2, 8, 0, 0, 2, REDUCE)),
    C(64, 3072, 1024, PLAIN, F16, Plan(STREAM, 4, 0, 0, 0, 1, 1, NONE)),
    C(57, 16392, 192, PLAIN, F32, Plan(WIDE, 4, 0, 0, 0, 0, 1, NONE)),
    C(64, 200, 192, PLAIN, F16, Plan(MID, 4, 0, 0, 0, 0, 1, NONE), norm=True),
    C(49, 96, 512, SILU, F16, Plan(MID, 4, 0, 0, 0, 0, 2, REDUCE), norm=True),
    C(65, 200, 192, PLAIN, F16, Plan(TILE, 0, 0, 0, 0, 0, 1, NONE)),
    C(3300, 5100, 1280, PLAIN, F32R, Plan(PP, 0, 0, 0, 0, 0, 5, PP_REDUCE)),
    C(3300, 5100, 1280, PLAIN, F32, Plan(PP, 0, 0, 0, 0, 0, 5, PP_REDUCE)),
    C(3300, 5100, 1280, GELU, F16, Plan(PP, 0, 0, 0, 0, 0, 5, PP_REDUCE)),
    C(3300, 5088, 1280, SILU, F16, Plan(PP, 0, 0, 0, 0, 0, 5, PP_REDUCE)),
    C(3000, 8100, 1536, PLAIN, F32, Plan(PP, 0, 0, 0, 0, 0, 2, PP_REDUCE)),
    C(3000, 8192, 1536, PLAIN, F16, Plan(PP, 0, 0, 0, 0, 0, 2, PP_PAIR)),
    C(3000, 8192, 1536, PLAIN, F32R, Plan(PP, 0, 0, 0, 0, 0, 2, PP_PAIR)),
    C(3000, 8192, 1536, GELU, F16, Plan(PP, 0, 0, 0, 0, 0, 2, PP_PAIR)),
    C(3000, 8192, 1536, SILU, F16, Plan(PP, 0, 0, 0, 0, 0, 2, PP_PAIR)),
]
SLAB_CASES = [
    C(20, 4608, 1024, PLAIN, F16, Plan(STREAM, 2, 0, 0, 0, 3, 2, SLABS), slab=True),
    C(20, 2048, 1024, PLAIN, F16, Plan(WIDE, 2, 0, 0, 0, 0, 2, SLABS), slab=True),
    C(37, 2048, 2048, PLAIN, F16, Plan(WIDE, 4, 0, 0, 0, 0, 4, SLABS), slab=True),
]
CASES = OLD_KERNEL_CASES + OLD_NORM_CASES + NEW_CASES


def case_id(c):
    tag = ("plain", "gelu", "silu")[c.epi] + "-" + c.mode + ("-norm" if c.norm else "") + ("-atiled" if c.a_tiled else "") + ("-slab" if c.slab else "")
    return f"{c.M}x{c.N}x{c.K}-{tag}"


def cell_of(c):
    p = c.plan
    return Cell(p.klass, p.mt, p.tn, p.ns, p.alds, p.P, c.norm, c.epi, c.mode, p.combine)


def route_case(c):
    return route(c.M, c.N, c.K, c.epi, c.mode, norm=c.norm, a_tiled=c.a_tiled, slab_only=c.slab)


def bf16_subset():
    """The cases the bf16 build repeats: per (kernel instantiation, fused norm, epilogue) the one whose k-parts take the longest way."""
    best = {}
    for c in NEW_CASES:
        key = cell_of(c)[:8]
        if key not in best or c.plan.combine > best[key].plan.combine:
            best[key] = c
    return list(best.values())


# ------------------------------------------------------------------------------------------------ inputs
# Exact family.  A and W hold the integers -7 .. 7 without 0 (dense: every k of every row carries weight), W scaled by 2^-e; bias
# and residual are integers in -64 .. 64 times 2^-e.  Every product, every partial sum in any order and the bias / residual
# additions are integers below 2^24 in units of 2^-e, hence exact in fp32 (EXACT_BOUND below, checked per case on the CPU), so the
# pre-activation does not depend on summation order, on k-part seams or on which workgroup arrives first.  The integers are exact in
# fp16 and in bf16 (3 significant bits).  e puts the standard deviation of the pre-activation, 20 sqrt(K) 2^-e (E[x^2] = 20 for
# either factor), at about 1, so that GELU and silu(g) u see |pre-activation| of a few units - PRE_RANGE, checked on the CPU.
A_MAX, W_MAX, B_MAX = 7, 7, 64
PRE_RANGE = 8.0
SENTINEL = -1024.0            # guard rows behind the output (exact in fp16, bf16 and fp32)
GUARD_ROWS = 8


def scale_exp(K):
    import math
    return round(math.log2(20.0 * math.sqrt(K)))


def exact_bound(K):
    """largest |partial sum| any order can reach, in units of 2^-e: sum |a| |w| + |bias| + |residual|"""
    return A_MAX * W_MAX * K + 2 * B_MAX


def _ints(shape, hi, g):
    v = torch.randint(1, hi + 1, shape, generator=g, dtype=torch.int8)
    return torch.where(torch.randint(0, 2, shape, generator=g, dtype=torch.int8) == 1, v, -v)


def exact_inputs(c):
    """(A int8 [M, K], W int8 [N, K], bias int8 [N], residual int8 [M, Nout] or None, e): the operands are these integers, W, bias and
    residual times 2^-e.  Generated on the CPU from the case alone."""
    g = torch.Generator().manual_seed(c.M * 1000003 + c.N * 1009 + c.K + 7 * c.epi)
    nout = c.N // 2 if c.epi == SILU else c.N
    A, W = _ints((c.M, c.K), A_MAX, g), _ints((c.N, c.K), W_MAX, g)
    bias = torch.randint(-B_MAX, B_MAX + 1, (c.N,), generator=g, dtype=torch.int8)
    res = torch.randint(-B_MAX, B_MAX + 1, (c.M, nout), generator=g, dtype=torch.int8) if c.mode == F32R else None
    return A, W, bias, res, scale_exp(c.K)


def activate(pre, epi):
    """fp64 of the epilogue on the [M, N] pre-activation (gate / up: 32-column groups [16 gate | 16 up])"""
    if epi == GELU:
        return torch.nn.functional.gelu(pre)
    if epi == SILU:
        M, N = pre.shape
        a = pre.view(M, N // 32, 2, 16)
        return (torch.nn.functional.silu(a[:, :, 0]) * a[:, :, 1]).reshape(M, N // 2)
    return pre


def exact_reference(A, W, bias, res, e, epi):
    """fp64 reference of the exact family on whatever device the operands live on: the matmul of these integers is exact in any order"""
    pre = (A.double() @ W.double().T + bias.double()) * 2.0 ** -e
    out = activate(pre, epi)
    return pre, (out if res is None else out + res.double() * 2.0 ** -e)


def gaussian_inputs(c):
    """The fused-norm family of tests/test_gpu_parity.py::test_gemm_fused_rmsnorm: X fp32 [M, K] ~ 3 N(0, 1), W ~ N(0, 1 / K)"""
    g = torch.Generator().manual_seed(c.M * 13 + c.N)
    return torch.randn(c.M, c.K, generator=g) * 3.0, torch.randn(c.N, c.K, generator=g) / c.K ** 0.5


def norm_reference(X, W16, epi, eps=1e-5):
    x = X.double()
    return activate((x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)) @ W16.double().T, epi)


def a_rows(M):
    """rows of the activation buffer: the M real ones, then NaN rows up to the largest row tile a kernel at this M works on"""
    return cdiv(M, 64) * 64 if M <= 64 else 128 if M <= 128 else cdiv(M, 256) * 256


KERNEL_RULE = (2e-3, 1e-5)         # tests/test_gpu_parity.py::test_gemm_kernels: 2e-3 max |ref| + 1e-5
NORM_RULE = (4e-3, 1e-5)           # ::test_gemm_fused_rmsnorm (the kernel rounds h, not h / rms, to fp16)
BF16_FACTOR = 8                    # tests/test_gpu_bf16.py: bf16 has 8 significand bits against fp16's 11
