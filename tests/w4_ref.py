"""CPU twin of the MXFP4 quantiser (csrc/quant.hip) and of the MXFP4 code / scale panel layout, in integer arithmetic on the fp32
bits of torch CPU tensors (tests/test_w4_host.py checks it against a brute-force fp64 search; tests/test_gpu_w4.py holds the kernel
to it bit for bit).  Not product code.

Format (OCP MX v1.0 MXFP4; W[N, K] in the operand type fp16 or bf16; a block is 32 consecutive k of one row):
  e     floor(log2(absmax_block)) - 2, from the fp32 exponent field of absmax_block (no log2); never below EXP_MIN; 0 for an all-zero
        block (and for an absmax below the smallest normal fp32: bf16 only).  Stored byte: e + 127 (e8m0)
  q     e2m1 code: magnitude RNE(min(|w| 2^-e, 6)) over VALUES with ties to the even code (5 -> 4), sign in bit 3; then +0 where
        q 2^e would be subnormal in the operand type, and +0 for a negative zero
  dq    q 2^e, exact in the operand type
Panels: tiled_off / scale_off below (mx4_code_off / mx4_scale_off of csrc/common.h).
"""
from __future__ import annotations

import torch

EXP_MIN = -120
VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)                    # the magnitudes of codes 0 .. 7
LIMITS = {torch.float16: (-14, 15), torch.bfloat16: (-126, 127)}     # binary exponents of the smallest normal / largest finite value
BLOCK = 32
# fp32 bit patterns of the decision points 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 and which side the tie goes to (True: up - the
# upper neighbour is the even code)
_CUTS = ((0x3E800000, False), (0x3F400000, True), (0x3FA00000, False), (0x3FE00000, True), (0x40200000, False), (0x40600000, True),
         (0x40A00000, False))
_XQ = torch.tensor([-1000, -1, 0, 0, 1, 1, 2, 2])                    # binary exponent of the magnitude of codes 0 .. 7


def e2m1_values() -> torch.Tensor:
    """fp64 value of every code 0 .. 15 (code 8 is -0.0)"""
    v = torch.tensor(VALUES, dtype=torch.float64)
    return torch.cat([v, -v])


def block_exponents(W: torch.Tensor) -> torch.Tensor:
    """int32 [N, K / 32] from the fp32 bit fields of the blocks' absmax (no log2)."""
    N, K = W.shape
    b = W.float().abs().reshape(N, K // BLOCK, BLOCK).amax(dim=2).view(torch.int32)
    e = ((b >> 23) - 127 - 2).clamp(min=EXP_MIN)
    return torch.where(b < 0x00800000, torch.zeros_like(e), e)


def rne_e2m1(vbits: torch.Tensor) -> torch.Tensor:
    """magnitude codes 0 .. 7 of non-negative fp32 values given by their bits (int64): nearest of VALUES, ties to the even code,
    saturating at 6 - by comparing bit patterns (non-negative floats order as their bits)"""
    m = torch.zeros_like(vbits)
    for cut, tie_up in _CUTS:
        m += (vbits >= cut) if tie_up else (vbits > cut)
    return m


def quantize(W: torch.Tensor):
    """(codes uint8 [N, K] row-major, values 0 .. 15; scale bytes uint8 [N, K / 32] row-major; dq in W's dtype) of a finite W."""
    assert W.dtype in LIMITS and W.dim() == 2 and W.shape[1] % BLOCK == 0
    if not torch.isfinite(W).all():
        raise ValueError("a weight is not finite")
    lo, hi = LIMITS[W.dtype]
    N, K = W.shape
    eb = block_exponents(W)
    e = eb.long().repeat_interleave(BLOCK, dim=1)
    bits = W.float().contiguous().view(torch.int32).long() & 0xFFFFFFFF
    sign, mag = bits >> 31, bits & 0x7FFFFFFF
    ex = mag >> 23
    live = (ex > 0) & (ex - e > 0)                                   # |w| 2^-e is a normal fp32 (below that it rounds to 0 anyway)
    m = torch.where(live, rne_e2m1(mag - (e << 23)), torch.zeros_like(mag))
    flush = (m == 0) | (_XQ[m] + e < lo)
    m = torch.where(flush, torch.zeros_like(m), m)
    q = torch.where(m > 0, m | (sign << 3), m).to(torch.uint8)
    dq64 = e2m1_values()[q.long()] * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())
    dq = dq64.to(W.dtype)
    assert torch.equal(dq.double(), dq64), "dq is not exact in the operand type"
    assert int((_XQ[m] + e)[m > 0].max() if bool((m > 0).any()) else lo) <= hi
    return q, (eb + 127).to(torch.uint8), dq


def dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp64 [N, K] of row-major codes and scale bytes"""
    return e2m1_values()[q.long()] * torch.pow(torch.tensor(2.0, dtype=torch.float64), s.double() - 127.0).repeat_interleave(BLOCK, dim=1)


# ------------------------------------------------------------------------------------------------ layout
def tiled_off(n: int, k: int, K: int):
    """(byte offset in the code panels of W[N, K], nibble) of element (n, k) (mx4_code_off, csrc/common.h)"""
    return ((n >> 4) * (K >> 6) + (k >> 6)) * 512 + ((((k & 31) >> 3) << 4) + (n & 15)) * 8 + ((k & 63) >> 5) * 4 + ((k & 7) >> 1), k & 1


def tiled_inv(off: int, nib: int, K: int):
    """(n, k) of nibble nib of byte offset off"""
    blk, r = divmod(off, 512)
    lane, b = divmod(r, 8)
    p, c = divmod(blk, K >> 6)
    return 16 * p + (lane & 15), 64 * c + 32 * (b >> 2) + 8 * (lane >> 4) + 2 * (b & 3) + nib


def scale_off(n: int, kb: int, K: int) -> int:
    """byte offset in the scale panels of the scale of block (n, kb = k / 32) (mx4_scale_off)"""
    return ((n >> 4) * (K >> 6) + (kb >> 1)) * 32 + (n & 15) * 2 + (kb & 1)


def scale_inv(off: int, K: int):
    blk, r = divmod(off, 32)
    p, c = divmod(blk, K >> 6)
    return 16 * p + (r >> 1), 2 * c + (r & 1)


def tile(q: torch.Tensor) -> torch.Tensor:
    """row-major codes [N, K] (0 .. 15) -> code panels uint8 [N, K / 2]"""
    N, K = q.shape
    x = q.reshape(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5)               # (p, c, g, li, k-step, j)
    return (x[..., 0::2] | (x[..., 1::2] << 4)).reshape(N, K // 2).contiguous()


def untile(t: torch.Tensor) -> torch.Tensor:
    N, K = t.shape[0], t.shape[1] * 2
    b = t.reshape(N // 16, K // 64, 4, 16, 2, 4)
    x = torch.stack((b & 15, b >> 4), dim=-1).reshape(N // 16, K // 64, 4, 16, 2, 8)
    return x.permute(0, 3, 1, 4, 2, 5).reshape(N, K).contiguous()


def tile_scales(s: torch.Tensor) -> torch.Tensor:
    """row-major scale bytes [N, K / 32] -> scale panels (same shape)"""
    N, KB = s.shape
    return s.reshape(N // 16, 16, KB // 2, 2).permute(0, 2, 1, 3).reshape(N, KB).contiguous()


def untile_scales(t: torch.Tensor) -> torch.Tensor:
    N, KB = t.shape
    return t.reshape(N // 16, KB // 2, 16, 2).permute(0, 2, 1, 3).reshape(N, KB).contiguous()


# ------------------------------------------------------------------------------------------------ inputs
def edge_rows(K: int, dtype) -> torch.Tensor:
    """Rows whose first block sits on the rules' edges, [R, K] in `dtype` (K >= 64): an absmax with mantissa 1.0 / 1.49 / 1.5 /
    1.99 at several binades, the smallest normal, one below it, the largest finite value, an all-zero block, a block whose small
    members flush, negative zeros; every block carries the planted ties and a spread of smaller magnitudes."""
    lo, hi = LIMITS[dtype]
    below = 2.0 ** lo * (1.0 - 2.0 ** (-10 if dtype == torch.float16 else -7))            # the largest subnormal
    biggest = (2.0 - 2.0 ** (-10 if dtype == torch.float16 else -7)) * 2.0 ** hi
    tops = [1.0, 1.4921875, 1.5, 1.9921875, 1.0 * 2.0 ** -5, 1.4921875 * 2.0 ** 3, 1.5 * 2.0 ** -9, 1.9921875 * 2.0 ** 6,
            2.0 ** lo, below, biggest, 0.0, 2.0 ** (lo + 2), 2.0 ** (lo + 3) * 1.5, 3.0e-3]
    g = torch.Generator().manual_seed(5)
    rows = []
    for t in tops:
        r = (torch.rand(K, generator=g, dtype=torch.float64) * 2 - 1) * t
        x = 2.0 ** (torch.floor(torch.log2(torch.tensor(t))).item() - 2) if t > 0 else 0.0   # 2^e of the first block
        for j, f in enumerate((0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, -0.25, -2.5, -5.0, 0.5, 6.0, -6.0, 0.2499, 5.01)):
            r[j + 1] = f * x
        r[0] = t
        r[17] = -0.0
        r[K - 1] = -t
        rows.append(r)
    return torch.stack(rows).to(dtype)
