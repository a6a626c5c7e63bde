"""CPU twin of the FP8 quantiser (csrc/quant.hip) and of the FP8 panel layout, in integer / exact float arithmetic on torch CPU
tensors (tests/test_w8_host.py checks it against torch.float8_e4m3fn; tests/test_gpu_w8.py holds the kernel to it bit for bit).
Not product code.

Format (per output row n of W[N, K], operand type fp16 or bf16):
  e_n   the smallest integer with absmax_n 2^-e_n <= 448 (= 1.75 2^8), from the exponent and mantissa fields of absmax_n;
        0 for an all-zero row (and for an absmax below the smallest normal fp32: bf16 only); never below EXP_MIN
  q     RNE_e4m3fn(W 2^-e_n), then +0 where q 2^e_n would be subnormal in the operand type, and the next code towards zero where
        rounding carried q 2^e_n past the operand type's largest finite value (fp16 |w| >= 63488)
  dq    q 2^e_n, exact in the operand type
"""
from __future__ import annotations

import torch

EXP_MIN = -120
E4M3_MAX = 448.0
LIMITS = {torch.float16: (-14, 15), torch.bfloat16: (-126, 127)}     # binary exponents of the smallest normal / largest finite value


def e4m3_values() -> torch.Tensor:
    """fp64 value of every code 0 .. 255 (NaN at 0x7f and 0xff), from the format's definition: 1 sign, 4 exponent (bias 7), 3
    mantissa bits, subnormals at exponent field 0, no infinities."""
    c = torch.arange(256)
    ex, m = (c >> 3) & 15, (c & 7).double()
    mag = torch.where(ex == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * torch.pow(torch.tensor(2.0, dtype=torch.float64), (ex - 7).double()))
    v = torch.where((c & 0x80) != 0, -mag, mag)
    v[0x7f] = v[0xff] = float("nan")
    return v


def row_exponents(W: torch.Tensor) -> torch.Tensor:
    """int8 [N] from the fp32 bit fields of the rows' absmax (no log2)."""
    a = W.float().abs().amax(dim=1)
    b = a.view(torch.int32)
    e = (b >> 23) - 127 - 8 + ((b & 0x7FFFFF) > 0x600000).int()
    e = torch.where(b < 0x00800000, torch.zeros_like(e), e.clamp(min=EXP_MIN))
    return e.to(torch.int8)


def rne_e4m3(x: torch.Tensor) -> torch.Tensor:
    """uint8 codes of fp32 x, |x| <= 448, round to nearest even - by integer arithmetic on the fp32 bits (no float8 dtype)."""
    b = x.float().contiguous().view(torch.int32).long() & 0xFFFFFFFF
    sign, mag = (b >> 24) & 0x80, b & 0x7FFFFFFF
    sub = torch.round(mag.int().view(torch.float32).double() * 512.0).long()          # torch.round: half to even; 0 .. 8
    nrm = ((mag + 0x7FFFF + ((mag >> 20) & 1)) >> 20) - ((127 - 7) << 3)
    return (sign | torch.where(mag < 0x3C800000, sub, nrm)).to(torch.uint8)


def quantize(W: torch.Tensor):
    """(codes uint8 [N, K] row-major, e int8 [N], dq in W's dtype) of a finite operand-type W."""
    assert W.dtype in LIMITS and W.dim() == 2
    if not torch.isfinite(W).all():
        raise ValueError("a weight is not finite")
    lo, hi = LIMITS[W.dtype]
    e = row_exponents(W)
    ef = e.double()[:, None]
    scaled = W.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -ef)       # exact: a power of two on <= 11 bits
    q = rne_e4m3(scaled.float())
    vals = e4m3_values()
    mag = vals[(q & 0x7F).long()]
    xq = torch.floor(torch.log2(mag.clamp(min=2.0 ** -20)))                           # (exact on 4-bit significands)
    over = (mag > 0) & (xq + ef > hi)
    q = torch.where(over, q - 1, q)
    mag = vals[(q & 0x7F).long()]
    xq = torch.floor(torch.log2(mag.clamp(min=2.0 ** -20)))
    flush = (mag == 0) | (xq + ef < lo)
    q = torch.where(flush, torch.zeros_like(q), q)
    dq64 = vals[q.long()] * torch.pow(torch.tensor(2.0, dtype=torch.float64), ef)
    dq = dq64.to(W.dtype)
    assert torch.equal(dq.double(), dq64), "dq is not exact in the operand type"
    return q, e, dq


def bits_to_half(b: torch.Tensor) -> torch.Tensor:
    """The bit form of the conversion: h = (b & 0x80) << 8 | (b & 0x7f) << 7 read as fp16 is value / 256 (uint8 codes in)."""
    b = b.to(torch.int32)
    h = ((b & 0x80) << 8) | ((b & 0x7F) << 7)
    return (h - ((h & 0x8000) << 1)).to(torch.int16).view(torch.float16)            # (the 16 bits as a signed int16)


def tiled_off(n: int, k: int, K: int) -> int:
    """byte offset of element (n, k) in the FP8 panels of W[N, K] (fp8_tiled_off, csrc/common.h)"""
    return ((n >> 4) * (K >> 6) + (k >> 6)) * 1024 + ((((k & 31) >> 3) << 4) + (n & 15)) * 16 + ((k & 63) >> 5) * 8 + (k & 7)


def tiled_inv(off: int, K: int):
    """(n, k) of byte offset off"""
    blk, r = divmod(off, 1024)
    lane, b = divmod(r, 16)
    p, c = divmod(blk, K >> 6)
    return 16 * p + (lane & 15), 64 * c + 32 * (b >> 3) + 8 * (lane >> 4) + (b & 7)


def tile(q: torch.Tensor) -> torch.Tensor:
    """row-major codes [N, K] -> FP8 panels (same shape, the bytes in panel order)"""
    N, K = q.shape
    return q.reshape(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(N, K).contiguous()


def untile(t: torch.Tensor) -> torch.Tensor:
    N, K = t.shape
    return t.reshape(N // 16, K // 64, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).reshape(N, K).contiguous()


def edge_rows(K: int, dtype) -> torch.Tensor:
    """Rows that sit on the rules' edges, [R, K] in `dtype` (K >= 64): per row an absmax and a spread of smaller magnitudes."""
    lo, hi = LIMITS[dtype]
    tops = [1.75, 1.75 * 2.0 ** -3, 1.7578125 if dtype == torch.float16 else 1.765625, 1.0, 1.9921875, 2.0 ** lo, 2.0 ** (lo + 3),
            0.0, 3.0e-3, 2.0 ** (hi - 4) * 1.5]
    if dtype == torch.float16:
        tops += [65504.0, 63488.0, 63456.0, 2.0 ** -24, 2.0 ** -15]
    rows = []
    g = torch.Generator().manual_seed(5)
    for t in tops:
        r = (torch.rand(K, generator=g, dtype=torch.float64) * 2 - 1) * t
        # ties of the 3-bit mantissa, a few binades down (exact in the operand type), and subnormal-range e4m3 values
        for j, f in enumerate((1.0625, 1.1875, 0.53125, 0.59375, 2.0 ** -14, 3 * 2.0 ** -16, 2.0 ** -17, 2.0 ** -18 * 1.5, -1.0625, -2.0 ** -16)):
            r[j + 1] = t * f / 1.75 if t else 0.0
        r[0] = t
        r[K - 1] = -t
        rows.append(r)
    return torch.stack(rows).to(dtype)
