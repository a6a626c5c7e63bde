"""Weights in HBM: fused layouts the kernels stream, built from the canonical (reference-named) tensors.

Replaces the state-dict loading of load_pretrained_model / initialize_protein_modules
(model/builder.py:60-65,107-111; model/opus_arch.py:81-90).  PyTorch owns the device memory; the
library borrows the pointers through opus_bind_weight.

Fused tensors (fp16 GEMM weights [out, in] = nn.Linear orientation, fp32 vectors):
  enc.emb [33,De] (row-major gather table) | enc.{l}.wqkv [3De,De] = [q;k;v] rows diag(ln1.weight),
  enc.{l}.bqkv [3De] = [q;k;v] bias + W ln1.bias, enc.{l}.sqkv = row sums of the folded wqkv | enc.{l}.wo,bo |
  enc.{l}.w1 = fc1 diag(ln2.weight), b1 = fc1.bias + W ln2.bias, s1 | enc.{l}.w2,b2 | enc.lnf.{w,b}
  proj.{w,b} | sw.{i}.{w,b}
  dec.emb [V,H] (row-major gather table) | dec.{l}.wqkv [(nh+2nkv)hd,H] | dec.{l}.wo
  dec.{l}.wgu [2F,H]: 32-row groups = [16 gate rows | 16 up rows] so that a 16-column MFMA tile of
  gate and its matching tile of up are produced by one workgroup (silu(g)*u in the epilogue)
  dec.{l}.wd [H,F] | dec.lm_head [V,H]
Two load-time transforms make the hot loop a pure stream:
  * every GEMM weight is stored PANEL-TILED (16-row x 64-k blocks in MFMA B-fragment order, see
    csrc/gemm.hip): one wave-wide 16-B load = 1 KB of contiguous HBM = one MFMA operand;
  * the decoder's RMSNorm weights are FOLDED into the projection that consumes the normalised
    activations (wqkv <- wqkv diag(input_norm), wgu <- wgu diag(post_norm), lm_head <- lm_head diag(norm)),
    fp32 product rounded once to fp16, so the kernels only need 1/rms(x) (computed in the GEMM prologue);
  * the encoder's pre-LayerNorms are folded the same way, LN(x) W^T + b = rstd (x W'^T - mu s) + c2 with W' = W diag(gamma),
    s[n] = sum_k W'[n][k] (of the ROUNDED W', so that the mean cancels exactly) and c2 = W beta + b in fp32: the kernels need
    (mu, rstd) per row only, either applied in the GEMM epilogue (csrc/gemm.hip gemm_pp_kernel, GemmParams::ln_*) or by the
    stand-alone normalisation (x - mu) rstd in front of a plain GEMM with bias c2.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _cabi, synth
from .config import OpusConfig


@dataclass(frozen=True)
class Part:
    canon: str       # canonical tensor name
    rows: int
    cols: int        # 1 for vectors
    rb: int          # row block
    rs: int          # destination rows per block
    ro: int          # destination row offset


@dataclass(frozen=True)
class Fused:
    name: str
    f16: bool
    shape: Tuple[int, ...]
    parts: Tuple[Part, ...]
    tiled: bool = False          # GEMM weight stored panel-tiled
    fold: Optional[str] = None   # canonical norm weight multiplied into the columns
    # derived fp32 vectors of a folded LayerNorm (see the module docstring):
    #   ("colsum", fused weight name)                       s[n] = sum_k W'[n][k] of the folded, rounded weight
    #   ("bias_fold", fused weight name, canonical LN bias)  parts (the Linear bias) + W beta, W the UNFOLDED weight
    derive: Optional[Tuple[str, ...]] = None


def _cat(name, f16, cols, pieces: List[Tuple[str, int]], tiled=False, fold=None) -> Fused:
    parts, off = [], 0
    for canon, rows in pieces:
        parts.append(Part(canon, rows, cols, rows, rows, off))
        off += rows
    shape = (off, cols) if f16 or cols > 1 else (off,)
    return Fused(name, f16, shape, tuple(parts), tiled, fold)


def fused_spec(cfg: OpusConfig) -> List[Fused]:
    De, Fe = cfg.enc_dim, cfg.enc_ffn
    H, F, V = cfg.dec_dim, cfg.dec_ffn, cfg.dec_vocab
    out: List[Fused] = []
    mat = lambda n, c, r, k, fold=None: out.append(_cat(n, True, k, [(c, r)], True, fold))   # noqa: E731
    tab = lambda n, c, r, k: out.append(_cat(n, True, k, [(c, r)]))       # noqa: E731  (row-major gather table)
    vec = lambda n, c, r: out.append(_cat(n, False, 1, [(c, r)]))         # noqa: E731
    tab("enc.emb", "enc.embed_tokens", cfg.enc_vocab, De)
    for l in range(cfg.enc_layers):
        s, d = f"enc.layers.{l}.", f"enc.{l}."
        out.append(_cat(d + "wqkv", True, De, [(s + "q.weight", De), (s + "k.weight", De), (s + "v.weight", De)], True,
                        s + "ln1.weight"))
        bq = _cat(d + "bqkv", False, 1, [(s + "q.bias", De), (s + "k.bias", De), (s + "v.bias", De)])
        out.append(Fused(bq.name, False, bq.shape, bq.parts, derive=("bias_fold", d + "wqkv", s + "ln1.bias")))
        out.append(Fused(d + "sqkv", False, (3 * De,), (), derive=("colsum", d + "wqkv")))
        mat(d + "wo", s + "o.weight", De, De); vec(d + "bo", s + "o.bias", De)
        mat(d + "w1", s + "fc1.weight", Fe, De, s + "ln2.weight")
        b1 = _cat(d + "b1", False, 1, [(s + "fc1.bias", Fe)])
        out.append(Fused(b1.name, False, b1.shape, b1.parts, derive=("bias_fold", d + "w1", s + "ln2.bias")))
        out.append(Fused(d + "s1", False, (Fe,), (), derive=("colsum", d + "w1")))
        mat(d + "w2", s + "fc2.weight", De, Fe); vec(d + "b2", s + "fc2.bias", De)
    vec("enc.lnf.w", "enc.ln_f.weight", De); vec("enc.lnf.b", "enc.ln_f.bias", De)
    if cfg.has_protein_projector:
        mat("proj.w", "proj.weight", cfg.proj_dim, De); vec("proj.b", "proj.bias", cfg.proj_dim)
    din = cfg.switch_in
    for i in range(cfg.switch_depth):
        mat(f"sw.{i}.w", f"switch.{i}.weight", cfg.switch_out, din); vec(f"sw.{i}.b", f"switch.{i}.bias", cfg.switch_out)
        din = cfg.switch_out
    tab("dec.emb", "dec.embed_tokens", V, H)
    if cfg.dec_arch == 1:       # OPT / Galactica: nothing folded (LayerNorm has a mean), biases kept as fp32 vectors
        tab("dec.pos", "dec.embed_positions", cfg.dec_max_pos + 2, H)
        for l in range(cfg.dec_layers):
            s, d = f"dec.layers.{l}.", f"dec.{l}."
            vec(d + "ln1.w", s + "ln1.weight", H); vec(d + "ln1.b", s + "ln1.bias", H)
            out.append(_cat(d + "wqkv", True, H, [(s + "q.weight", cfg.dec_q_dim), (s + "k.weight", cfg.dec_kv_dim),
                                                 (s + "v.weight", cfg.dec_kv_dim)], True))
            out.append(_cat(d + "bqkv", False, 1, [(s + "q.bias", cfg.dec_q_dim), (s + "k.bias", cfg.dec_kv_dim),
                                                  (s + "v.bias", cfg.dec_kv_dim)]))
            mat(d + "wo", s + "o.weight", H, cfg.dec_q_dim); vec(d + "bo", s + "o.bias", H)
            vec(d + "ln2.w", s + "ln2.weight", H); vec(d + "ln2.b", s + "ln2.bias", H)
            mat(d + "w1", s + "fc1.weight", F, H); vec(d + "b1", s + "fc1.bias", F)
            mat(d + "w2", s + "fc2.weight", H, F); vec(d + "b2", s + "fc2.bias", H)
        vec("dec.lnf.w", "dec.norm.weight", H); vec("dec.lnf.b", "dec.norm.bias", H)
        mat("dec.lm_head", "dec.lm_head.weight", V, H)
        return out
    for l in range(cfg.dec_layers):
        s, d = f"dec.layers.{l}.", f"dec.{l}."
        out.append(_cat(d + "wqkv", True, H, [(s + "q.weight", cfg.dec_q_dim), (s + "k.weight", cfg.dec_kv_dim),
                                             (s + "v.weight", cfg.dec_kv_dim)], True, s + "input_norm.weight"))
        if cfg.dec_qkv_bias:    # Qwen2: the bias is added after the (folded-norm) projection, so it is not folded
            out.append(_cat(d + "bqkv", False, 1, [(s + "q.bias", cfg.dec_q_dim), (s + "k.bias", cfg.dec_kv_dim),
                                                  (s + "v.bias", cfg.dec_kv_dim)]))
        mat(d + "wo", s + "o.weight", H, cfg.dec_q_dim)
        out.append(Fused(d + "wgu", True, (2 * F, H), (Part(s + "gate.weight", F, H, 16, 32, 0),
                                                       Part(s + "up.weight", F, H, 16, 32, 16)),
                         True, s + "post_norm.weight"))
        mat(d + "wd", s + "down.weight", H, F)
    mat("dec.lm_head", "dec.lm_head.weight", V, H, "dec.norm.weight")
    return out


def _dst_rows(p: Part, device) -> torch.Tensor:
    r = torch.arange(p.rows, device=device)
    return (r // p.rb) * p.rs + p.ro + (r % p.rb)


def tile_weight(t: torch.Tensor) -> torch.Tensor:
    """Row-major fp16 [N,K] on the GPU -> panel-tiled copy (same nominal shape) via opus_tile_weight."""
    assert t.is_cuda and t.dtype == _cabi.operand_dtype() and t.dim() == 2 and t.is_contiguous()
    out = torch.empty_like(t)
    with torch.cuda.device(t.device):
        _cabi.check(_cabi.lib().opus_tile_weight(t.data_ptr(), out.data_ptr(), t.shape[0], t.shape[1],
                                                 torch.cuda.current_stream(t.device).cuda_stream))
    return out


def untile_weight(t: torch.Tensor) -> torch.Tensor:
    """Inverse of tile_weight (host-side index arithmetic; tests and debugging only)."""
    N, K = t.shape
    return t.reshape(N // 16, K // 64, 2, 4, 16, 8).permute(0, 4, 1, 2, 3, 5).reshape(N, K).contiguous()


def _quantize_via(entry: str, t: torch.Tensor, codes_cols: int, scales_shape: Tuple[int, ...], scales_dtype: torch.dtype):
    """(codes uint8 [N, codes_cols], scales, dq: the dequantised weights in the operand type, row-major) of a row-major
    operand-type [N,K] on the GPU via the library's `entry`.  Raises OpusError when a weight is not finite."""
    assert t.is_cuda and t.dtype == _cabi.operand_dtype() and t.dim() == 2 and t.is_contiguous()
    N, K = t.shape
    codes = torch.empty((N, codes_cols), dtype=torch.uint8, device=t.device)
    scales = torch.empty(scales_shape, dtype=scales_dtype, device=t.device)
    dq = torch.empty_like(t)
    with torch.cuda.device(t.device):
        _cabi.check(getattr(_cabi.lib(), entry)(t.data_ptr(), N, K, codes.data_ptr(), scales.data_ptr(), dq.data_ptr(),
                                                torch.cuda.current_stream(t.device).cuda_stream))
    return codes, scales, dq


def quantize_fp8(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Row-major operand-type [N,K] on the GPU -> (q8 uint8 [N,K]: e4m3fn codes in the FP8 panel layout, e8 int8 [N]: the row
    exponents, dq: q 2^e in the operand type, row-major) via opus_quantize_fp8.  Raises OpusError when a weight is not finite."""
    return _quantize_via("opus_quantize_fp8", t, t.shape[1], (t.shape[0],), torch.int8)


def untile_fp8(q8: torch.Tensor) -> torch.Tensor:
    """FP8 panels [N,K] -> the codes row-major (host-side index arithmetic; tests and debugging only)."""
    N, K = q8.shape
    return q8.reshape(N // 16, K // 64, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).reshape(N, K).contiguous()


def quantize_mxfp4(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Row-major operand-type [N,K] on the GPU -> (q4 uint8 [N,K/2]: packed e2m1 codes in the MXFP4 code panels, s4 uint8 [N,K/32]:
    the e8m0 block scales in the scale panels, dq: q 2^e in the operand type, row-major) via opus_quantize_mxfp4.  Raises OpusError
    when a weight is not finite."""
    return _quantize_via("opus_quantize_mxfp4", t, t.shape[1] // 2, (t.shape[0], t.shape[1] // 32), torch.uint8)


def untile_mxfp4(q4: torch.Tensor, s4: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """MXFP4 code panels [N,K/2] and scale panels [N,K/32] -> (the codes 0 .. 15 row-major uint8 [N,K], the scale bytes row-major
    uint8 [N,K/32]) (host-side index arithmetic; tests and debugging only)."""
    N, K = q4.shape[0], q4.shape[1] * 2
    b = q4.reshape(N // 16, K // 64, 4, 16, 2, 4)
    codes = torch.stack((b & 15, b >> 4), dim=-1).reshape(N // 16, K // 64, 4, 16, 2, 8)
    codes = codes.permute(0, 3, 1, 4, 2, 5).reshape(N, K).contiguous()
    scales = s4.reshape(N // 16, K // 64, 16, 2).permute(0, 2, 1, 3).reshape(N, K // 32).contiguous()
    return codes, scales


@dataclass(frozen=True)
class WeightFormat:
    """One quantised form of the decoder layers' projections: `quantize(t)` -> (codes, scales, dequantised weights), the suffixes
    the code and scale tensors are bound under with their _cabi dtype codes, and the two values of `decoder_weights` that select
    it - `keyword` keeps the panels for the decode step, `keyword_dequantized` the dequantised tensors alone."""
    quantize: Callable[[torch.Tensor], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]
    suffixes: Tuple[Tuple[str, int], Tuple[str, int]]
    keyword: str
    keyword_dequantized: str


WEIGHT_FORMATS = (
    WeightFormat(quantize_fp8, ((".q8", _cabi.OPUS_F8E4M3), (".e8", _cabi.OPUS_I8)), "fp8", "fp8_dequantized"),
    # OCP MXFP4 (e2m1 codes, one e8m0 scale per 32 k of a row)
    WeightFormat(quantize_mxfp4, ((".q4", _cabi.OPUS_F4E2M1X2), (".s4", _cabi.OPUS_E8M0)), "mxfp4", "mxfp4_dequantized"),
)
DECODER_WEIGHT_FORMATS = (None,) + tuple(k for f in WEIGHT_FORMATS for k in (f.keyword, f.keyword_dequantized))


def quantized_names(cfg: OpusConfig) -> List[str]:
    """The fused tensors a quantised `decoder_weights` format quantises: the four projections of every decoder layer (lm_head, the
    embeddings, the encoder and the projectors stay as they are)."""
    mats = ("wqkv", "wo", "w1", "w2") if cfg.dec_arch == 1 else ("wqkv", "wo", "wgu", "wd")
    return [f"dec.{l}.{m}" for l in range(cfg.dec_layers) for m in mats]


class DeviceWeights:
    """Fused weight tensors on one GPU + their binding to a library context."""

    def __init__(self, cfg: OpusConfig, device: torch.device):
        self.cfg = cfg
        self.device = device
        self.decoder_weights: Optional[str] = None       # None | "fp8" | "fp8_dequantized" | "mxfp4" | "mxfp4_dequantized" (from_canonical / synthetic)
        self.tensors: Dict[str, torch.Tensor] = {}
        # optional tensors bound beside the fused ones (the ESM-2 contact head: enc.contact.weight fp32 [enc_layers * enc_heads],
        # enc.contact.bias fp32 [1]; the ESM-2 masked-LM head: enc.lm.*); opus_weights_ready does not need them
        self.extra: Dict[str, torch.Tensor] = {}

    CONTACT_NAMES = ("enc.contact.weight", "enc.contact.bias")

    def set_contact_head(self, weight, bias) -> None:
        """Bind the contact regression (canonical names enc.contact.{weight,bias}) at the next bind()."""
        C = self.cfg.enc_layers * self.cfg.enc_heads
        w = torch.as_tensor(np.asarray(weight) if not torch.is_tensor(weight) else weight).float().reshape(-1)
        b = torch.as_tensor(np.asarray(bias) if not torch.is_tensor(bias) else bias).float().reshape(-1)
        if w.numel() != C or b.numel() != 1:
            raise ValueError(f"contact head: weight [{C}] and bias [1] expected, got {tuple(w.shape)} and {tuple(b.shape)}")
        self.extra["enc.contact.weight"] = w.to(self.device).contiguous()
        self.extra["enc.contact.bias"] = b.to(self.device).contiguous()

    MLM_NAMES = synth.MLM_HEAD_NAMES          # (+ the optional enc.lm.weight of an untied output projection)

    def set_mlm_head(self, head: Dict[str, "np.ndarray | torch.Tensor"]) -> None:
        """Bind the masked-LM head (canonical names enc.lm.dense.{weight,bias}, enc.lm.ln.{weight,bias}, enc.lm.bias and,
        when the output projection is not tied to enc.embed_tokens, enc.lm.weight) at the next bind(): the two matrices in the
        build's operand type (the dense one panel-tiled for the GEMM kernels, the output table row-major), the vectors in fp32."""
        De, V = self.cfg.enc_dim, self.cfg.enc_vocab
        missing = [k for k in self.MLM_NAMES if k not in head]
        if missing:
            raise ValueError(f"masked-LM head: {missing} missing")
        shapes = {"enc.lm.dense.weight": (De, De), "enc.lm.dense.bias": (De,), "enc.lm.ln.weight": (De,), "enc.lm.ln.bias": (De,),
                  "enc.lm.bias": (V,), "enc.lm.weight": (V, De)}
        new = {}
        with torch.cuda.device(self.device):
            for k, sh in shapes.items():
                if k not in head:
                    continue
                t = head[k]
                t = torch.as_tensor(np.asarray(t)) if not torch.is_tensor(t) else t
                if tuple(t.shape) != sh:
                    raise ValueError(f"masked-LM head: {k} has shape {tuple(t.shape)}, expected {sh}")
                mat = len(sh) == 2
                t = t.to(self.device).to(_cabi.operand_dtype() if mat else torch.float32).contiguous()
                new[k] = tile_weight(t) if k == "enc.lm.dense.weight" else t
        self.extra.pop("enc.lm.weight", None)
        self.extra.update(new)

    def has_mlm_head(self) -> bool:
        return all(k in self.extra for k in self.MLM_NAMES)

    # -- construction -------------------------------------------------------------------------
    def _alloc(self, f: Fused) -> torch.Tensor:
        t = torch.empty(f.shape, dtype=_cabi.operand_dtype() if f.f16 else torch.float32, device=self.device)
        self.tensors[f.name] = t
        return t

    @classmethod
    def from_canonical(cls, cfg: OpusConfig, canon: Dict[str, "np.ndarray | torch.Tensor"], device,
                       lora: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor, float, int]]] = None,
                       decoder_weights: Optional[str] = None) -> "DeviceWeights":
        """Canonical tensors (reference parameter names, see synth.py) -> fused device tensors.

        `lora` maps a canonical weight name to (A [r,in], B [out,r], alpha, r): merged into that weight
        first, W += (alpha / r) B A, as peft merge_and_unload does at model/builder.py:107-109 (row L1).
        `decoder_weights`: one of DECODER_WEIGHT_FORMATS (_quantize below).
        """
        self = cls(cfg, torch.device(device))
        self._set_decoder_weights(decoder_weights)
        lib = _cabi.lib()

        def get(name, dtype):
            v = canon[name]
            v = torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v
            return v.to(self.device).to(dtype)

        spec = fused_spec(cfg)
        # bias_fold entries need W @ beta of the weight BEFORE its fold: computed the moment that weight is assembled and kept as a
        # vector (holding every unfolded fp32 weight until _derive ran was ~1.5 GB of transient memory for ESM-2 650M, 6.6 GB for 3B)
        wanted = {f.derive[1]: f.derive[2] for f in spec if f.derive and f.derive[0] == "bias_fold"}
        folded_vec: Dict[str, torch.Tensor] = {}
        with torch.cuda.device(self.device):
            for f in spec:
                t = self._alloc(f)
                t2 = t.view(t.shape[0], -1)
                for p in f.parts:
                    src = get(p.canon, t.dtype).reshape(p.rows, p.cols).contiguous()
                    if lora and p.canon in lora:
                        A, B, alpha, r = lora[p.canon]
                        A = A.to(self.device, _cabi.operand_dtype()).contiguous()
                        B = B.to(self.device, _cabi.operand_dtype()).contiguous()
                        _cabi.check(lib.opus_lora_merge(src.data_ptr(), A.data_ptr(), B.data_ptr(), float(alpha) / float(r),
                                                        p.rows, p.cols, int(r), torch.cuda.current_stream().cuda_stream))
                    t2[_dst_rows(p, self.device)] = src
                if f.name in wanted:
                    folded_vec[f.name] = t.float() @ get(wanted[f.name], torch.float32)
                if f.fold is not None:
                    t.copy_((t.float() * get(f.fold, torch.float32)[None, :]).to(_cabi.operand_dtype()))
                if f.name in self._quantized_names:
                    t = self._quantize(f.name, t)
                if f.tiled:
                    self.tensors[f.name] = tile_weight(t)
            self._derive(spec, None, None, folded_vec)
            if all(k in canon for k in self.CONTACT_NAMES):
                self.set_contact_head(canon["enc.contact.weight"], canon["enc.contact.bias"])
            if all(k in canon for k in self.MLM_NAMES):
                self.set_mlm_head({k: v for k, v in canon.items() if k.startswith("enc.lm.")})
            torch.cuda.synchronize(self.device)
        return self

    def _set_decoder_weights(self, decoder_weights: Optional[str]) -> None:
        if decoder_weights not in DECODER_WEIGHT_FORMATS:
            raise ValueError(f"decoder_weights={decoder_weights!r}: one of {DECODER_WEIGHT_FORMATS}")
        self.decoder_weights = decoder_weights
        self._quantized_names = set(quantized_names(self.cfg)) if decoder_weights else set()

    def _quantize(self, name: str, t: torch.Tensor) -> torch.Tensor:
        """The quantised form (self.decoder_weights, a row of WEIGHT_FORMATS) of the fused decoder-layer weight `name` (row-major,
        after LoRA merge, concatenation / interleave and norm fold, before tiling), csrc/quant.hip.  FP8: per-row power-of-two
        exponent + e4m3fn codes.  MXFP4: e2m1 codes with one power-of-two scale per 32 consecutive k of a row.  Returns the
        dequantised weights (exactly representable in the operand type), which take the weight's place, so prefill, forward,
        scoring and every decode launch without a kernel for the format compute with the same numbers.  The panels-kept keyword
        ("fp8", "mxfp4") also keeps the codes and scales, bound as `name` + the format's suffixes (.q8 / .e8, .q4 / .s4) for the
        decode step (Llama / Qwen2; OPT / Galactica run on the dequantised tensors); the "_dequantized" keyword keeps the
        dequantised tensors alone (the comparison model).
        MXFP4 is uncalibrated round-to-nearest: ~11 % relative rms error per row on Gaussian weights - a different model, and a
        decode-throughput option that ADDS 0.27 x the decoder-layer weights in memory."""
        fmt = next(f for f in WEIGHT_FORMATS if self.decoder_weights in (f.keyword, f.keyword_dequantized))
        codes, scales, dq = fmt.quantize(t.contiguous())
        if self.decoder_weights == fmt.keyword and self.cfg.dec_arch == 0:
            self.tensors[name + fmt.suffixes[0][0]], self.tensors[name + fmt.suffixes[1][0]] = codes, scales
        return dq

    @property
    def decoder_weight_format(self) -> str:
        return self.decoder_weights or ("bf16" if _cabi.BF16 else "fp16")

    def _derive(self, spec, unfolded, vector, folded_vec=None) -> None:
        """The derived vectors of the folded LayerNorms (Fused.derive): unfolded(name) -> fp32 [N, K] row-major weight before
        the fold, vector(canonical name) -> fp32 vector; or folded_vec[name] = that weight @ its vector, already computed."""
        for f in spec:
            if not f.derive:
                continue
            t = self.tensors[f.name]
            if f.derive[0] == "colsum":
                t.copy_(untile_weight(self.tensors[f.derive[1]]).float().sum(dim=1))
            elif f.derive[0] == "bias_fold":
                t.add_(folded_vec[f.derive[1]] if folded_vec is not None else unfolded(f.derive[1]) @ vector(f.derive[2]))
            else:
                raise ValueError(f.derive)

    @classmethod
    def synthetic(cls, cfg: OpusConfig, seed: int, device, stream: int = 0, contact_head: bool = False,
                  mlm_head: bool = False, decoder_weights: Optional[str] = None) -> "DeviceWeights":
        """Fill the fused tensors on the GPU with the deterministic synthetic model (synth.py twin); contact_head: also the
        synthetic contact regression (synth.contact_head); mlm_head: also the synthetic masked-LM head (synth.mlm_head);
        decoder_weights: one of DECODER_WEIGHT_FORMATS (_quantize)."""
        self = cls(cfg, torch.device(device))
        self._set_decoder_weights(decoder_weights)
        lib = _cabi.lib()
        if not stream:      # the fills and _derive's torch ops on ONE stream: torch's current one (not the null stream beside it)
            stream = torch.cuda.current_stream(self.device).cuda_stream
        spec = {n: (sh, std, mean) for n, sh, std, mean in synth.canonical_spec(cfg)}
        fspec = fused_spec(cfg)
        by_name = {f.name: f for f in fspec}

        def fill(t, f16, p: Part, tiled, fold=(0, 0.0, 0.0)):
            _, std, mean = spec[p.canon]
            _cabi.check(lib.opus_fill_synth(t.data_ptr(), _cabi.OPUS_F16 if f16 else _cabi.OPUS_F32, p.rows, p.cols,
                                            synth.tensor_seed(p.canon, seed), std, mean, p.rb, p.rs, p.ro, 1 if tiled else 0,
                                            fold[0], fold[1], fold[2], stream))

        def unfolded(name):          # the fused weight `name` before the fold, row-major fp32 (a temporary of at most a few MB)
            f = by_name[name]
            tmp = torch.empty(f.shape, dtype=_cabi.operand_dtype(), device=self.device)
            for p in f.parts:
                fill(tmp, True, p, False)
            return tmp.float()

        def vector(canon_name):
            sh, _, _ = spec[canon_name]
            tmp = torch.empty(sh, dtype=torch.float32, device=self.device)
            fill(tmp, False, Part(canon_name, int(sh[0]), 1, int(sh[0]), int(sh[0]), 0), False)
            return tmp

        with torch.cuda.device(self.device), torch.cuda.stream(torch.cuda.ExternalStream(stream) if stream else torch.cuda.current_stream()):
            for f in fspec:
                t = self._alloc(f)
                fseed, fstd, fmean = 0, 0.0, 0.0
                if f.fold is not None:
                    _, fstd, fmean = spec[f.fold]
                    fseed = synth.tensor_seed(f.fold, seed)
                for p in f.parts:
                    _, std, mean = spec[p.canon]
                    _cabi.check(lib.opus_fill_synth(t.data_ptr(), _cabi.OPUS_F16 if f.f16 else _cabi.OPUS_F32,
                                                    p.rows, p.cols, synth.tensor_seed(p.canon, seed), std, mean,
                                                    p.rb, p.rs, p.ro, 1 if f.tiled else 0, fseed, fstd, fmean, stream))
                if f.name in self._quantized_names:      # (filled panel-tiled: back to rows, quantise, tile the dequantised weights)
                    self.tensors[f.name] = tile_weight(self._quantize(f.name, untile_weight(t)))
            self._derive(fspec, unfolded, vector)
            if contact_head:
                head = synth.contact_head(cfg, seed)
                self.set_contact_head(head["enc.contact.weight"], head["enc.contact.bias"])
            if mlm_head:
                self.set_mlm_head(synth.mlm_head(cfg, seed))
        return self

    # -- binding ---------------------------------------------------------------------------------
    def bind(self, ctx) -> None:
        lib = _cabi.lib()
        quantized = {sfx: code for f in WEIGHT_FORMATS for sfx, code in f.suffixes}     # (the code and scale tensors, by suffix)
        for name, t in list(self.tensors.items()) + list(self.extra.items()):
            shape = (C.c_int64 * t.dim())(*t.shape)
            _cabi.check(lib.opus_bind_weight(ctx, name.encode(), t.data_ptr(),
                                             _cabi.OPUS_F16 if t.dtype == _cabi.operand_dtype() else
                                             quantized.get(name[-3:], _cabi.OPUS_F32),
                                             t.dim(), shape))
        _cabi.check(lib.opus_weights_ready(ctx))

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in list(self.tensors.values()) + list(self.extra.values()))
