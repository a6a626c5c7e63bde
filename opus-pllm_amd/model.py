"""Host-side mirror of the reference's model interface for the multi_modality_v1 inference path.

Same names, argument meaning and error behaviour as
  multi_modality_v1/model/language_model/opus_llama.py  (OpusLlamaForCausalLM.generate :95-132)
  multi_modality_v1/model/opus_arch.py                  (encode_* :103-131,
                                                          prepare_inputs_labels_for_multimodal :133-294)
so that eval/run_opus_ddp.py-style callers drop in.  Every tensor op of the path runs in
libopus_pllm.so; PyTorch only owns device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import types
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _cabi
from .alphabet import batch_convert, batch_convert_packed, encode_array, pack_token_arrays
from .config import OpusConfig
from .constants import DEFAULT_SEQ_TOKEN_INDEX, IGNORE_INDEX
from .weights import DeviceWeights

TOP_LOGPROBS_MAX = 20          # generate() / forward()'s top_logprobs (csrc/common.h: TOPK_MAX)


class _ProteinEncoderHandle:
    """What get_protein_encoder() returns: exposes get_protein_seq_embeddings like
    ProteinSeqEmbeddingExtractor (cstp_v3/modelling.py:37)."""

    def __init__(self, owner: "OpusLlamaForCausalLM"):
        self._owner = owner

    def get_protein_seq_embeddings(self, data: Sequence[str]) -> torch.Tensor:
        return self._owner._encode(list(data))

    def get_amino_acid_embeddings(self, data, return_contacts: bool = False):
        """ProteinSeqEmbeddingExtractor.get_amino_acid_embeddings (cstp_v3/modelling.py:61-77): data = [(label, sequence)] (or
        plain sequences) -> list of fp32 [n_i, enc_dim] per-residue last-layer states (rows 1 .. len_i - 2 of
        representations[enc_layers], as the reference slices them at :75) on the model's device; with return_contacts=True
        (embeddings, contacts), contacts a list of fp32 [n_i, n_i] maps equal to fair-esm's results["contacts"][i, :n_i, :n_i].
        The reference feeds CPU tokens to the model it moved to the GPU (:35 vs :68), so its call as written fails with a device
        mismatch; this is the intended behaviour."""
        seqs = [d[1] if isinstance(d, (tuple, list)) else d for d in data]
        return self._owner._amino_acid_embeddings(seqs, return_contacts)

    def get_residue_logits(self, data, log_softmax: bool = False):
        """The masked-LM head's logits per residue: data = [(label, sequence)] (or plain sequences, which may contain <mask>) ->
        list of fp32 [n_i, 33] on the model's device, row j = residue j of protein i (the <cls> / <eos> rows are dropped), equal to
        fair-esm's model(tokens)["logits"][i, 1 : n_i + 1] and transformers' EsmForMaskedLM; log_softmax=True: their log-softmax
        over the 33 columns.  One packed encoder call per max_batch proteins, the head on the residue rows only."""
        seqs = [d[1] if isinstance(d, (tuple, list)) else d for d in data]
        return self._owner._residue_logits(seqs, log_softmax)

    def score_mutations(self, data, mutations=None, mode: str = "masked-marginals", positions=None, offset_idx: int = 1):
        """Variant-effect scores as fair-esm's examples/variant-prediction/predict.py computes them -> mlm.MutationScores.
        mode "wt-marginals": one pass over the unmasked sequences; "masked-marginals": row j from the copy whose residue j is
        <mask> (the host builds the copies, max_batch per encoder call, copies of different proteins share a call, the head runs
        on one gathered row per copy).  positions: per protein the 0-based residues to scan (default: all, or with mutations
        the ones they mention).  mutations: per protein a list of strings such as "A23G" or "A23G:L40P" (positions count from
        offset_idx; a multiple mutation is the sum of its parts); a string that does not fit its protein raises ValueError."""
        seqs = [d[1] if isinstance(d, (tuple, list)) else d for d in data]
        return self._owner._score_mutations(seqs, mutations, mode, positions, offset_idx)


class _InnerModel:
    """What get_model() returns (OpusLlamaModel in the reference): embed_tokens + module handles."""

    def __init__(self, owner: "OpusLlamaForCausalLM"):
        self._owner = owner
        self.config = owner.config
        self.protein_encoder = _ProteinEncoderHandle(owner)

    def get_protein_encoder(self):
        return self.protein_encoder

    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        return torch.nn.functional.embedding(ids.to(self._owner.device), self._owner.weights.tensors["dec.emb"])


class OpusLlamaForCausalLM:
    """MI355X-native stand-in for the reference's OpusLlamaForCausalLM (inference only)."""

    def __init__(self, cfg: OpusConfig, weights: DeviceWeights, device: Union[str, torch.device] = "cuda:0",
                 eos_token_id: Union[int, Sequence[int], None] = None, pad_token_id: Optional[int] = None):
        self.cfg = cfg.validate()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _cabi.OpusError(-102, "OpusLlamaForCausalLM needs a GPU device: there is no CPU path")
        self.weights = weights
        self._lib = _cabi.lib()
        self._ctx = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        cc = _cabi.CConfig.from_config(cfg)
        _cabi.check(self._lib.opus_ctx_create(C.byref(cc), idx, C.byref(self._ctx)))
        weights.bind(self._ctx)
        self._stream = torch.cuda.Stream(self.device)
        self.config = types.SimpleNamespace(
            hidden_size=cfg.dec_dim, vocab_size=cfg.dec_vocab, has_switch_projector=True, has_protein_encoder=True,
            num_hidden_layers=cfg.dec_layers, device=str(self.device), model_type="opus_llama")
        eos = [] if eos_token_id is None else ([eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id))
        self.generation_config = types.SimpleNamespace(eos_token_id=eos, pad_token_id=pad_token_id)
        self.model = _InnerModel(self)

    # ------------------------------------------------------------------ lifecycle
    def new_context(self) -> "OpusLlamaForCausalLM":
        """A second context on the same device that SHARES this model's weights (read-only) and owns its workspace, KV cache,
        decode graph and stream: two batches can then be in flight on one GPU (two host threads, one per context) - proteins are
        independent, so one batch's kernels stream through the other's launch gaps, ramps and drains - mostly in the decode steps
        (`eval_ddp.py --inflight 2`, `bench.py`'s `two_in_flight`: +10 % throughput at batch 64; same ids as one context)."""
        g = self.generation_config
        return OpusLlamaForCausalLM(self.cfg, self.weights, self.device, eos_token_id=list(g.eos_token_id), pad_token_id=g.pad_token_id)

    @property
    def decoder_weight_format(self) -> str:
        """What the decoder layers' projections are bound as: "fp16" / "bf16" (the build's operand type, unquantised), "fp8" (FP8
        panels for the decode step beside the dequantised operand-type tensors), "fp8_dequantized" (those tensors alone), "mxfp4" or
        "mxfp4_dequantized" (the same with MXFP4 code and scale panels)."""
        return self.weights.decoder_weight_format

    def __del__(self):
        try:
            if getattr(self, "_ctx", None) and self._ctx.value:
                self._lib.opus_ctx_destroy(self._ctx)
                self._ctx = C.c_void_p()
        except Exception:
            pass

    def eval(self):
        return self

    def get_model(self):
        return self.model

    def get_protein_encoder(self):
        return self.model.get_protein_encoder()

    # ------------------------------------------------------------------ stream plumbing
    def _enter(self):
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        return self._stream.cuda_stream

    def _leave(self):
        torch.cuda.current_stream(self.device).wait_stream(self._stream)

    # ------------------------------------------------------------------ rows E0-E4
    packed_encoder = True      # token-packed (varlen) encoder; False: the padded, length-bucketed form (A/B and parity tests)

    def _encode(self, seqs: List[str], bucket: int = 256) -> torch.Tensor:
        """list[str] -> pooled fp32 [B, enc_dim].  Token-packed by default: the proteins' tokens go through the encoder back to
        back with no padding and no buckets (opus_esm2_encode_packed), max_batch proteins per call."""
        if self.packed_encoder:
            return self._encode_packed(seqs)
        return self._encode_padded(seqs, bucket)

    def _encode_packed(self, seqs: List[str]) -> torch.Tensor:
        cfg = self.cfg
        n = len(seqs)
        out = torch.empty((n, cfg.enc_dim), dtype=torch.float32, device=self.device)
        s = self._enter()
        keep = []
        for i0 in range(0, n, cfg.max_batch):
            toks, cu = batch_convert_packed(seqs[i0:i0 + cfg.max_batch])
            B = len(cu) - 1
            longest = int((cu[1:] - cu[:-1]).max())
            if longest > cfg.max_enc_tokens:
                raise _cabi.OpusError(-2, f"protein of {longest - 2} residues exceeds max_enc_tokens={cfg.max_enc_tokens}")
            with torch.cuda.stream(self._stream):
                d_tok = torch.from_numpy(toks).to(self.device, non_blocking=True)
                cu_arr = (C.c_int32 * (B + 1))(*[int(v) for v in cu])
                _cabi.check(self._lib.opus_esm2_encode_packed(self._ctx, d_tok.data_ptr(), cu_arr, B, out[i0:].data_ptr(), s))
            keep.append(d_tok)
            self._last_enc_shape = (1, int(cu[-1]))
        self._leave()
        return out

    # caller scratch of one contacts call (opus_esm2_contacts_scratch_bytes): proteins are grouped so that a group stays under this
    # many bytes (a single protein may exceed it alone: 4000 residues at the ESM-2 650M shape need about 64 MB of map + 21 MB of
    # per-channel vectors + the column partials)
    CONTACT_SCRATCH_BUDGET = 1 << 30

    def _amino_acid_embeddings(self, seqs: List[str], return_contacts: bool = False):
        cfg = self.cfg
        cc = _cabi.CConfig.from_config(cfg)
        embs: List[torch.Tensor] = []
        maps: List[torch.Tensor] = []
        n = len(seqs)
        i0 = 0
        s = self._enter()
        try:
            while i0 < n:
                i1 = min(n, i0 + cfg.max_batch)
                toks, cu = batch_convert_packed(seqs[i0:i1])
                longest = int((cu[1:] - cu[:-1]).max())
                if longest > cfg.max_enc_tokens:
                    raise _cabi.OpusError(-2, f"protein of {longest - 2} residues exceeds max_enc_tokens={cfg.max_enc_tokens}")
                if return_contacts:
                    while True:         # shrink the group until its scratch fits the budget (or it is one protein)
                        B = len(cu) - 1
                        cu_arr = (C.c_int32 * (B + 1))(*[int(v) for v in cu])
                        need = int(self._lib.opus_esm2_contacts_scratch_bytes(C.byref(cc), cu_arr, B))
                        if need <= self.CONTACT_SCRATCH_BUDGET or B == 1:
                            break
                        i1 = i0 + max(1, B // 2)
                        toks, cu = batch_convert_packed(seqs[i0:i1])
                B = len(cu) - 1
                cu_arr = (C.c_int32 * (B + 1))(*[int(v) for v in cu])
                M = int(cu[-1])
                pooled = torch.empty((B, cfg.enc_dim), dtype=torch.float32, device=self.device)
                hidden = torch.empty((M, cfg.enc_dim), dtype=torch.float32, device=self.device)
                if return_contacts:
                    nres = (cu[1:] - cu[:-1] - 2).astype(np.int64)
                    out = torch.empty((max(1, int((nres * nres).sum())),), dtype=torch.float32, device=self.device)
                    scratch = torch.empty((max(need, 256),), dtype=torch.uint8, device=self.device)
                with torch.cuda.stream(self._stream):
                    d_tok = torch.from_numpy(toks).to(self.device, non_blocking=True)
                    if return_contacts:
                        _cabi.check(self._lib.opus_esm2_contacts_packed(self._ctx, d_tok.data_ptr(), cu_arr, B, pooled.data_ptr(),
                                                                        out.data_ptr(), scratch.data_ptr(), need, s))
                        off = 0
                        for nb in nres.tolist():
                            maps.append(out[off:off + nb * nb].view(nb, nb))
                            off += nb * nb
                    else:
                        _cabi.check(self._lib.opus_esm2_encode_packed(self._ctx, d_tok.data_ptr(), cu_arr, B, pooled.data_ptr(), s))
                    _cabi.check(self._lib.opus_esm2_last_hidden(self._ctx, hidden.data_ptr(), 1, M, s))
                    for b in range(B):
                        embs.append(hidden[int(cu[b]) + 1:int(cu[b + 1]) - 1])
                    self._last_enc_shape = (1, M)
                    if return_contacts:
                        scratch.record_stream(self._stream)
                    d_tok.record_stream(self._stream)
                i0 = i1
        finally:
            self._leave()
        return (embs, maps) if return_contacts else embs

    # ------------------------------------------------------------------ masked-LM head
    def _need_mlm_head(self) -> None:
        w = self.weights
        if not w.has_mlm_head():
            raise ValueError("no masked-LM head is bound: it is read from the ESM-2 checkpoint's lm_head.{dense,layer_norm}.{weight,bias}, "
                             "lm_head.weight and lm_head.bias (builder.mlm_head_from_esm2, the checkpoint OPUS_ESM2_CKPT names), or "
                             "made by DeviceWeights.synthetic(..., mlm_head=True) / DeviceWeights.set_mlm_head")
        key = tuple(w.extra[k].data_ptr() for k in w.MLM_NAMES) + (w.extra["enc.lm.weight"].data_ptr() if "enc.lm.weight" in w.extra else 0,)
        if getattr(self, "_mlm_bound", None) != key:      # (a head set after this context was made: bind it now)
            w.bind(self._ctx)
            self._mlm_bound = key

    def _mlm_rows(self, encs: List[np.ndarray], rows: List[Sequence[int]], log_softmax: bool):
        """Token arrays (residue ids, no <cls> / <eos>) through the packed encoder, max_batch per call, and the head on residue
        rows `rows[i]` (0-based) of each -> (list of fp32 [len(rows[i]), enc_vocab], encoder calls, rows evaluated)."""
        cfg = self.cfg
        V = cfg.enc_vocab
        outs: List[torch.Tensor] = []
        calls = nrows = 0
        s = self._enter()
        try:
            for i0 in range(0, len(encs), cfg.max_batch):
                group = encs[i0:i0 + cfg.max_batch]
                toks, cu = pack_token_arrays(group)
                B = len(cu) - 1
                longest = int((cu[1:] - cu[:-1]).max())
                if longest > cfg.max_enc_tokens:
                    raise _cabi.OpusError(-2, f"protein of {longest - 2} residues exceeds max_enc_tokens={cfg.max_enc_tokens}")
                idx = np.concatenate([np.asarray(rows[i0 + b], dtype=np.int32).reshape(-1) + np.int32(int(cu[b]) + 1) for b in range(B)])
                R = int(idx.size)
                out = torch.empty((R, V), dtype=torch.float32, device=self.device)
                if R:
                    cu_arr = (C.c_int32 * (B + 1))(*[int(v) for v in cu])
                    pooled = torch.empty((B, cfg.enc_dim), dtype=torch.float32, device=self.device)
                    with torch.cuda.stream(self._stream):
                        d_tok = torch.from_numpy(toks).to(self.device, non_blocking=True)
                        d_idx = torch.from_numpy(idx).to(self.device, non_blocking=True)
                        _cabi.check(self._lib.opus_esm2_encode_packed(self._ctx, d_tok.data_ptr(), cu_arr, B, pooled.data_ptr(), s))
                        _cabi.check(self._lib.opus_esm2_lm_head(self._ctx, d_idx.data_ptr(), R, 1 if log_softmax else 0, out.data_ptr(), s))
                        for t in (d_tok, d_idx, pooled, out):
                            t.record_stream(self._stream)
                    self._last_enc_shape = (1, int(cu[-1]))
                    calls += 1
                    nrows += R
                off = 0
                for b in range(B):
                    k = len(rows[i0 + b])
                    outs.append(out[off:off + k])
                    off += k
        finally:
            self._leave()
        return outs, calls, nrows

    def _residue_logits(self, seqs: List[str], log_softmax: bool = False):
        self._need_mlm_head()
        encs = [encode_array(q) for q in seqs]
        return self._mlm_rows(encs, [np.arange(len(e), dtype=np.int32) for e in encs], log_softmax)[0]

    def _score_mutations(self, seqs: List[str], mutations=None, mode: str = "masked-marginals", positions=None, offset_idx: int = 1):
        from . import mlm
        if mode not in mlm.MODES:
            raise ValueError(f"mode must be one of {mlm.MODES}, got {mode!r}")
        self._need_mlm_head()
        cfg = self.cfg
        encs = [encode_array(q) for q in seqs]
        P = len(encs)
        for name, v in (("mutations", mutations), ("positions", positions)):
            if v is not None and len(v) != P:
                raise ValueError(f"{name} holds {len(v)} lists for {P} proteins")
        parsed = None if mutations is None else [[mlm.parse_mutation(m, encs[i], offset_idx) for m in mutations[i]] for i in range(P)]
        lens = [len(e) for e in encs]
        scan = mlm.scan_positions(lens, positions, parsed)
        if mode == "wt-marginals":
            got, calls, nrows = self._mlm_rows(encs, scan, True)
        else:
            plan = mlm.plan_masked_copies(scan, lens, cfg.max_batch, cfg.max_enc_tokens)
            copies = [c for call in plan for c in call]
            got, calls, nrows = self._mlm_rows([mlm.masked_copy(encs[i], j) for i, j in copies], [[j] for _, j in copies], True)
        # one table over all proteins' residues (NaN where not scanned), its wild-type column and the sums in a handful of
        # launches; the per-protein results are views of it
        V = cfg.enc_vocab
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        N = int(offs[-1])
        rows = np.concatenate([np.asarray(scan[i], dtype=np.int64).reshape(-1) + offs[i] for i in range(P)]) if P else np.zeros(0, np.int64)
        flat = torch.cat(got, 0) if got else torch.empty((0, V), dtype=torch.float32, device=self.device)
        if rows.size == N:                    # every row scanned (ascending, no repeats): the table as it stands
            LP = flat
        else:
            LP = torch.full((N, V), float("nan"), dtype=torch.float32, device=self.device)
            if rows.size:
                LP[torch.from_numpy(rows).to(self.device)] = flat
        tok = torch.from_numpy(np.concatenate(encs).astype(np.int64) if N else np.zeros(0, np.int64)).to(self.device)
        WT = LP.gather(1, tok[:, None])[:, 0]
        SC = LP - WT[:, None]
        # per-protein sums through a padded [P, longest] matrix: a fixed summation order (no atomics), one launch
        seg = torch.from_numpy(np.repeat(np.arange(P, dtype=np.int64), lens)).to(self.device)
        pos = torch.from_numpy((np.arange(N, dtype=np.int64) - np.repeat(offs[:-1], lens))).to(self.device)
        pad = torch.zeros((P, max(lens, default=0) or 1), dtype=torch.float32, device=self.device)
        pad[seg, pos] = torch.nan_to_num(WT, nan=0.0)
        pll = pad.sum(1)
        cnt = torch.tensor([float(len(ps)) for ps in scan], dtype=torch.float32, device=self.device)
        res = mlm.MutationScores(mode, [], [], [], None, None, None if parsed is None else [], nrows, calls, scan)
        for i in range(P):
            a, b = int(offs[i]), int(offs[i + 1])
            res.log_probs.append(LP[a:b])
            res.wt_log_prob.append(WT[a:b])
            res.scores.append(SC[a:b])
            if parsed is not None:
                res.mutation_scores.append(torch.stack([sum(res.scores[i][idx, mt] for idx, _, mt in mut) for mut in parsed[i]])
                                           if parsed[i] else LP.new_empty((0,)))
        res.pseudo_log_likelihood = pll
        res.pseudo_perplexity = torch.exp(-pll / cnt)
        return res

    def _encode_padded(self, seqs: List[str], bucket: int = 256) -> torch.Tensor:
        """list[str] -> pooled fp32 [B, enc_dim].  Mixed lengths are processed in length buckets
        (multiples of `bucket` residues) so padding never exceeds one bucket; per-protein results do
        not depend on the batch they ran in (key padding is masked).  256 measured best on 64 proteins of
        128-1024 residues (363 ms per batch vs 399 ms at 64 and 381 ms unbucketed): fewer, larger GEMMs
        outweigh the extra padding."""
        cfg = self.cfg
        n = len(seqs)
        out = torch.empty((n, cfg.enc_dim), dtype=torch.float32, device=self.device)
        order = sorted(range(n), key=lambda i: len(seqs[i]))
        groups: List[List[int]] = []
        for i in order:
            key = (len(seqs[i]) + bucket - 1) // bucket
            if groups and groups[-1][0] == key and len(groups[-1][1]) < cfg.max_batch:
                groups[-1][1].append(i)
            else:
                groups.append([key, [i]])
        s = self._enter()
        keep = []
        for _, idxs in groups:
            toks, lens = batch_convert([seqs[i] for i in idxs])
            if toks.shape[1] < 3:       # only empty strings: <cls><eos> + one pad column (their mean over zero residues
                import numpy as np      # is NaN, as in the reference; such rows carry no <seq> placeholder)
                from .alphabet import PAD_IDX
                toks = np.concatenate([toks, np.full((toks.shape[0], 1), PAD_IDX, dtype=toks.dtype)], axis=1)
            B, T = toks.shape
            if T > cfg.max_enc_tokens:
                raise _cabi.OpusError(-2, f"protein of {T - 2} residues exceeds max_enc_tokens={cfg.max_enc_tokens}")
            with torch.cuda.stream(self._stream):
                d_tok = torch.from_numpy(toks).to(self.device, non_blocking=True)
                d_len = torch.from_numpy(lens).to(self.device, non_blocking=True)
                pooled = torch.empty((B, cfg.enc_dim), dtype=torch.float32, device=self.device)
                _cabi.check(self._lib.opus_esm2_encode(self._ctx, d_tok.data_ptr(), d_len.data_ptr(), B, T,
                                                       pooled.data_ptr(), s))
                out[torch.tensor(idxs, device=self.device)] = pooled
            keep.append((d_tok, d_len, pooled))
        self._leave()
        self._last_enc_shape = (B, T)
        return out

    def encode_seq2embedding(self, seq) -> torch.Tensor:
        """opus_arch.py:103-114: str | list[str] -> fp32 [B, enc_dim]; other types: NotImplementedError."""
        if type(seq) is not list:
            seq = [seq]
        if type(seq[0]) is str:
            return self.get_protein_encoder().get_protein_seq_embeddings(seq)
        raise NotImplementedError

    def encode_projector_embedding(self, extractor_embedding: torch.Tensor) -> torch.Tensor:
        """opus_arch.py:115-121 -> CSTPBase.protein_forward (modelling.py:396-400): fp16 [B, proj_dim].  Without a CSTP
        checkpoint the reference installs an identity module (opus_arch.py:70-80): the input comes back unchanged."""
        if not self.cfg.has_protein_projector:
            return extractor_embedding
        x = extractor_embedding.to(self.device, torch.float32).contiguous()
        B = x.shape[0]
        s = self._enter()
        with torch.cuda.stream(self._stream):
            y = torch.empty((B, self.cfg.switch_in), dtype=_cabi.operand_dtype(), device=self.device)
            _cabi.check(self._lib.opus_protein_projector(self._ctx, x.data_ptr(), B, y.data_ptr(), s))
        self._leave()
        return y

    def switch_projector_embedding(self, seq_embedding: torch.Tensor) -> torch.Tensor:
        """opus_arch.py:122-131: [B, switch_in] -> fp16 [B, n_prot_tokens, hidden]."""
        y = seq_embedding.to(self.device, _cabi.operand_dtype()).contiguous()
        B = y.shape[0]
        s = self._enter()
        with torch.cuda.stream(self._stream):
            z = torch.empty((B, self.cfg.n_prot_tokens, self.cfg.dec_dim), dtype=_cabi.operand_dtype(), device=self.device)
            _cabi.check(self._lib.opus_switch_projector(self._ctx, y.data_ptr(), B, z.data_ptr(), s))
        self._leave()
        return z

    # ------------------------------------------------------------------ rows S1-S3
    def _splice(self, input_ids, attention_mask, prot, inference_mode):
        cfg = self.cfg
        ids = input_ids.to(self.device, torch.int64).contiguous()
        B, Tt = ids.shape
        m = None if attention_mask is None else attention_mask.to(self.device).bool().to(torch.uint8).contiguous()
        prot = prot.to(self.device, _cabi.operand_dtype()).contiguous()
        s = self._enter()
        with torch.cuda.stream(self._stream):
            emb = torch.empty((B, cfg.max_prompt, cfg.dec_dim), dtype=_cabi.operand_dtype(), device=self.device)
            mo = torch.empty((B, cfg.max_prompt), dtype=torch.uint8, device=self.device)
            po = torch.empty((B, cfg.max_prompt), dtype=torch.int32, device=self.device)
            T_out = C.c_int32(0)
            max_len = int(getattr(self.config, "tokenizer_model_max_length", None) or 0)
            _cabi.check(self._lib.opus_splice_pad(self._ctx, ids.data_ptr(), None if m is None else m.data_ptr(), B, Tt,
                                                  prot.data_ptr(), prot.shape[0], 1 if inference_mode else 0, max_len,
                                                  emb.data_ptr(), mo.data_ptr(), po.data_ptr(), C.byref(T_out), s))
            T = T_out.value
            # the kernel wrote [B, T] densely at the head of the capacity-sized buffers
            emb = emb.view(-1)[: B * T * cfg.dec_dim].view(B, T, cfg.dec_dim)
            mo = mo.view(-1)[: B * T].view(B, T)
            po = po.view(-1)[: B * T].view(B, T)
        self._leave()
        return emb, mo, po

    PROJECT_CHUNK = 4096       # rows per projector launch of project_dataset (8H x 8H GEMM at 1.3 PFLOP/s from ~1024 rows up)

    def project_dataset(self, pooled: torch.Tensor) -> torch.Tensor:
        """The batched projector stage of the two-stage pipeline: pooled ESM-2 embeddings of a whole dataset
        shard fp32 [N, enc_dim] (the `input_embed` field written by generate_esm_embedding.py, consumed by the reference at
        opus_arch.py:151-161) -> protein tokens fp16 [N, n_prot_tokens, hidden], the modality projectors running at
        M = PROJECT_CHUNK rows (MFMA-bound GEMMs) instead of re-streaming their 2.5 GB of weights for every batch of 8.
        Every launch has the SAME shape - the last chunk is padded with zero rows - so a row's tokens (and the greedy ids that
        follow) do not depend on the shard size, i.e. on the number of ranks the dataset is split over.
        Feed slices of the result to generate(protein_tokens=...)."""
        x = pooled.to(self.device, torch.float32).contiguous()
        N, C_ = x.shape[0], self.PROJECT_CHUNK
        s = self._enter()
        with torch.cuda.stream(self._stream):
            z = torch.empty((N, self.cfg.n_prot_tokens, self.cfg.dec_dim), dtype=_cabi.operand_dtype(), device=self.device)
            zc = None
            for r0 in range(0, N, C_):
                n = min(C_, N - r0)
                if n == C_:
                    _cabi.check(self._lib.opus_projector_forward(self._ctx, x[r0:].data_ptr(), C_, z[r0:].data_ptr(), None, s))
                    continue
                xc = torch.zeros((C_, x.shape[1]), dtype=torch.float32, device=self.device)
                xc[:n] = x[r0:]
                zc = torch.empty((C_,) + tuple(z.shape[1:]), dtype=_cabi.operand_dtype(), device=self.device)
                _cabi.check(self._lib.opus_projector_forward(self._ctx, xc.data_ptr(), C_, zc.data_ptr(), None, s))
                z[r0:] = zc[:n]
        self._leave()
        return z

    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels,
                                             seq, seq_embedding=None, inference_mode=False, protein_tokens=None):
        """opus_arch.py:133-294.  Returns (None, position_ids|None, attention_mask|None, past_key_values,
        inputs_embeds [B,T,H] fp16, labels|None); inputs unchanged when seq is None or T == 1.
        protein_tokens (an extension, see project_dataset): already projected [n, n_prot_tokens, hidden] blocks."""
        if seq is None or self.get_protein_encoder() is None or input_ids.shape[1] == 1:
            return input_ids, position_ids, attention_mask, past_key_values, None, labels
        if protein_tokens is not None:
            seq_embedding = protein_tokens
        else:
            if seq_embedding is None:
                seq_embedding = self.encode_seq2embedding(seq)
            seq_embedding = self.encode_projector_embedding(seq_embedding)
            if self.config.has_switch_projector:
                seq_embedding = self.switch_projector_embedding(seq_embedding)
        if seq_embedding.ndimension() == 2:
            seq_embedding = seq_embedding.unsqueeze(1)
        elif seq_embedding.ndimension() != 3:
            raise NotImplementedError
        emb, mask_out, pos_out = self._splice(input_ids, attention_mask, seq_embedding, inference_mode)
        new_labels = None
        if labels is not None:
            new_labels = _splice_labels(input_ids, attention_mask, labels, self.cfg.n_prot_tokens, emb.shape[1],
                                        inference_mode).to(labels.device)
        out_mask = None if attention_mask is None else mask_out.to(dtype=attention_mask.dtype)
        out_pos = None if position_ids is None else pos_out.to(dtype=position_ids.dtype)
        return None, out_pos, out_mask, past_key_values, emb, new_labels

    # BASELINE.json's north_star calls the method by its short name; the reference defines only the long one (opus_arch.py:133)
    prepare_inputs_for_multimodal = prepare_inputs_labels_for_multimodal

    # ------------------------------------------------------------------ rows G0, G1, D1-D4
    @torch.no_grad()
    def generate(self, inputs: Optional[torch.Tensor] = None, seq=None, seq_embedding=None, **kwargs):
        """opus_llama.py:95-132 + GenerationMixin greedy search: returns ONLY the new ids [B, n_new].

        return_dict_in_generate=True returns a GenerateDecoderOnlyOutput (greedy, sampling) or a GenerateBeamDecoderOnlyOutput
        (num_beams > 1: `sequences`, `sequences_scores`) instead, `sequences` holding those same ids.  Without it the output_*
        flags are ignored, as in transformers.  Greedy and sampling only:
          output_scores: `scores`, one fp32 [B, V] device tensor per step - HF's processed scores (greedy: the logits; sampling:
            logits / temperature, -inf where top-k / top-p removed the token - the set the draw used);
          output_logits: `logits`, the raw fp32 logits per step (greedy: the same tensors as `scores`);
          output_token_logprobs (extension): `token_logprobs` fp32 [B, n] (log-probability of the chosen token under the
            model's distribution, 0 after a row finished; its EOS / last stop-sequence token counts), `logprob` [B] (row
            sums), `n_tokens` [B] (positions counted) - no [B, V] tensor is kept per step.
        Logits processors (greedy and sampling; transformers' semantics and order, before the sampling warpers):
        repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length / min_new_tokens (see _logits_processors).  They see
        only the ids generated so far, never the prompt, as the reference's generate from inputs_embeds does.  With any of them on,
        `scores` hold the processed scores while `logits` and `token_logprobs` stay raw; num_beams > 1 raises.
        Sampling warpers (do_sample=True; ignored otherwise, as in transformers): min_p, typical_p, epsilon_cutoff, eta_cutoff, in
        transformers' order behind temperature / top_k / top_p, min_tokens_to_keep = 1, on the GPU inside the captured step (see
        _sampling_warpers; off: None, and 0 / 1.0 / 0 / 0).  typical_p keeps a band of probabilities and can drop the most probable
        token; `scores` hold l / T on the kept set, `logits` and `token_logprobs` stay raw.  Bad values raise transformers'
        ValueErrors, num_beams > 1 with one of them on NotImplementedError.
        Constrained decoding (greedy and sampling): prefix_allowed_tokens_fn=TokenTrie(...) / TokenTrie.per_row([...])
        (constraint.py) - transformers' PrefixConstrainedLogitsProcessor as a device automaton, behind min_new_tokens and in front
        of the warpers; `scores` are -inf outside the allowed set, `logits` and `token_logprobs` stay raw.  Any other callable
        raises NotImplementedError (a Python callback cannot run inside the captured decode step), and so does num_beams > 1.
        num_return_sequences=N (transformers' semantics and row layout): with do_sample=True the result has B N rows, row b N + j
        the j-th sample of prompt b (`_expand_inputs_for_generation`).  The proteins are encoded and projected and the prompts
        prefilled ONCE, on B rows; the prefill leaves B N decoder rows (opus_llama_prefill_fanout) and the decode loop is that of
        a B N-row batch, the draw of row r at step t keyed by (seed, r, t).  Every output is [B N, ...]; EOS ids, the stop
        sequence, the processors and a TokenTrie act per decoder row, and TokenTrie.per_row of B tries gives row r trie r // N.
        `seq`, `seq_embedding` and `protein_tokens` carry B entries.  With num_beams=K >= N the N best finished hypotheses of
        every prompt come back best first ([B N, n], `sequences_scores` [B N]); the beams' prefill stays on B K rows.  Greedy
        search with N > 1, N > num_beams and N < 1 raise ValueError as transformers does; B N > max_batch raises OpusError.
        N = 1 (or absent) is the call without the argument.
        prefix=OpusPrefix (extension; cache_prefix()): `inputs` [R, n] are SUFFIX ids behind the cached prompt, left-padded or
        unpadded with attention_mask as always; they may hold <seq> placeholders with seq / seq_embedding / protein_tokens.  Row r
        continues prefix row prefix_rows[r] (any order, repeats; default the identity when R == prefix.rows).  The prefix is not
        run again: its K / V are placed under the R decode rows (kv_place_kernel) and only the suffix positions are prefilled;
        the decode loop, its graph and every option above act as for an R-row batch of the concatenated prompts.  A detached
        handle (cache_prefix(detach=True) / OpusPrefix.detach()) can be used any number of times, also from new_context()
        contexts; a live one is detached on the fly (one export) and is stale afterwards, as after any prefill.
        num_return_sequences=N with sampling expands the rows on the host (row r N + j), so the suffix pass runs N times per
        row.  num_beams > 1 raises NotImplementedError, an empty suffix row ValueError, a capacity violation OpusError -2.
        guidance_scale=g (transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor; greedy and sampling): classifier-free
        guidance against a negative prompt.  A call of P prompts runs 2 P decoder rows - rows [0, P) the prompts as always, rows
        [P, 2 P) the negative prompts, text only - so it costs about a plain call of 2 P rows.  Per step, in transformers' order:
        scores = g (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond) in fp32, then the logits processors, the
        TokenTrie, temperature / top-k / top-p, the arg-max or the draw on the P rows; the negative row decodes the token chosen for
        its prompt (pad ids once that row finished).  EOS ids, the stop sequence, processor histories and trie states
        (TokenTrie.per_row of P tries) belong to the P rows; every output has P rows, `scores` the guided, processed scores,
        `logits` and `token_logprobs` raw and conditional.  negative_prompt_ids [P, Tn] (+ negative_prompt_attention_mask;
        left-padded or unpadded) is used as given and may hold no <seq> placeholder; None (an extension: transformers has no
        default when it generates from embeddings) takes the call's own prompt with every <seq> placeholder dropped - the
        protein-free twin - so the answer is contrasted with what the text alone would say.  Both sets are left-padded to one
        length for the single 2 P-row prefill.  g None or 1 is the call without the argument (the negative prompt is ignored, as in
        transformers).  g not a finite number, a negative prompt of another row count or with a placeholder raise ValueError;
        2 P > max_batch or a padded length above max_prompt OpusError -2; num_beams > 1, num_return_sequences > 1 and prefix=
        with guidance NotImplementedError.
        prompt_lookup_num_tokens=k (transformers' prompt-lookup decoding; greedy search only, exact: the ids are those of the call
        without it): per pass every row drafts up to k ids by n-gram lookup in its own history (max_matching_ngram_size, default
        2: transformers' PromptLookupCandidateGenerator rule) and one pass of the decoder verifies all drafts, 1 + the longest
        draft positions per row; the rows accept in lockstep (the shortest accepted prefix over the unfinished rows), so a pass
        emits 1 + a ids per row for about the cost of one decode step.  The history is the text prompt (protein blocks are
        never matched), the ids generated so far and lookup_ids (extension: [B, L] ids or B id lists searched like the prompt -
        a retrieved annotation, an earlier answer, a term list).  batch x (k + 1) <= max_batch, else ValueError.  With
        return_dict_in_generate the result carries `stats` (LookupStats: passes, plain_steps, drafted, accepted).  do_sample,
        num_beams > 1, num_return_sequences > 1, guidance_scale, prefix=, the logits processors, a TokenTrie and the output_*
        flags raise NotImplementedError.  k None or 0 is the call without the argument.
        return_prefix=True (extension; needs return_dict_in_generate=True, else ValueError): the output's `prefix` is a DETACHED
        OpusPrefix of every row's prompt + answer, cut out of the cache the decode loop leaves (opus_llama_prefix_export_rows, one
        launch) - the next turn of a conversation is generate(follow_up_ids, prefix=out.prefix) and prefills the follow-up only.
        Row b emitted n_b ids (counted_tokens: up to and including its EOS id / the stop sequence's last id, else all); the
        handle holds K / V of the prompt and ids[b, : n_b - 1], `lengths` the rows' slot counts, `slots` their maximum, and
        `pending` (int64 [B]) ids[b, n_b - 1] - chosen but never fed.  generate(prefix=) and cache_prefix(prefix=) feed the
        pending id in front of the suffix (an empty suffix row is legal then); score_continuations / score_trie / search_trie
        want a sealed handle: cache_prefix(empty_rows, prefix=handle).  Works for greedy and sampling, with EOS ids, the stop
        sequence, the processors, a TokenTrie, the warpers and the output_* flags, behind plain generate() and generate(prefix=).
        num_beams > 1, num_return_sequences > 1, guidance_scale and prompt_lookup_num_tokens raise NotImplementedError.  The
        conversation has to fit max_prompt (prefix.slots + suffix <= max_prompt), else OpusError -2 naming the max_prompt needed."""
        return_dict = bool(kwargs.pop("return_dict_in_generate", False))
        want = {k: bool(kwargs.pop(k, False)) for k in ("output_scores", "output_logits", "output_token_logprobs",
                                                         "output_attentions", "output_hidden_states")}
        top_lp = _top_logprobs_arg(kwargs.pop("top_logprobs", None), getattr(getattr(self, "cfg", None), "dec_vocab", None))
        if not return_dict:
            top_lp = 0                                         # (ignored without the output object, as the output_* flags are)
        if return_dict:
            for k in ("output_attentions", "output_hidden_states"):
                if want[k]:
                    raise NotImplementedError(f"generate({k}=True) is not supported: the decode path keeps no per-layer tensors")
        kwargs.pop("position_ids", None)
        protein_tokens = kwargs.pop("protein_tokens", None)
        attention_mask = kwargs.pop("attention_mask", None)
        prefix = kwargs.pop("prefix", None)
        prefix_rows = kwargs.pop("prefix_rows", None)
        return_prefix = bool(kwargs.pop("return_prefix", False))
        guidance = _guidance_scale(kwargs.pop("guidance_scale", None))
        neg_ids = kwargs.pop("negative_prompt_ids", None)
        neg_mask = kwargs.pop("negative_prompt_attention_mask", None)
        lookup_k = kwargs.pop("prompt_lookup_num_tokens", None)
        lookup_k = int(lookup_k) if lookup_k else 0                      # (None / 0: the call without the argument)
        lookup_m = kwargs.pop("max_matching_ngram_size", None)
        lookup_ids = kwargs.pop("lookup_ids", None)
        if "inputs_embeds" in kwargs:
            raise NotImplementedError("`inputs_embeds` is not supported")
        do_sample = bool(kwargs.pop("do_sample", False))
        temperature = kwargs.pop("temperature", None)
        top_p = kwargs.pop("top_p", None)
        top_k = kwargs.pop("top_k", self.default_top_k)                  # (transformers 4.46.3: GenerationConfig.top_k = 50)
        seed = kwargs.pop("seed", None)
        num_beams = kwargs.pop("num_beams", 1)
        num_beams = 1 if num_beams is None else int(num_beams)
        if return_dict and num_beams > 1 and (want["output_scores"] or want["output_logits"] or want["output_token_logprobs"] or top_lp):
            raise NotImplementedError("with num_beams > 1, return_dict_in_generate returns `sequences` and `sequences_scores` only: "
                                      "output_scores / output_logits / output_token_logprobs / top_logprobs are built for greedy and sampling")
        nret = kwargs.pop("num_return_sequences", 1)
        nret = 1 if nret is None else int(nret)
        if nret < 1:
            raise ValueError(f"`num_return_sequences` has to be an integer strictly greater than 0 (got {nret})")
        if num_beams <= 1 and not do_sample and nret != 1:     # (GenerationConfig.validate's messages)
            raise ValueError("Greedy methods without beam search do not support `num_return_sequences` different than 1 "
                             f"(got {nret}).")
        if num_beams > 1 and nret > num_beams:
            raise ValueError(f"`num_return_sequences` ({nret}) has to be smaller or equal to `num_beams` ({num_beams}).")
        max_new = int(kwargs.pop("max_new_tokens", 32))
        kwargs.pop("use_cache", None)
        self.set_stop_sequence(kwargs.pop("stop_sequence", None))          # extension (opt-in "###" early stop), see below
        pad_id = kwargs.pop("pad_token_id", self.generation_config.pad_token_id)
        eos = kwargs.pop("eos_token_id", self.generation_config.eos_token_id)
        eos = [] if eos is None else ([int(eos)] if isinstance(eos, int) else [int(e) for e in eos])
        vocab = getattr(getattr(self, "cfg", None), "dec_vocab", None)
        lproc = _logits_processors(kwargs, eos, vocab)
        warpers = _sampling_warpers(kwargs)
        if not do_sample:
            warpers = None                                     # (transformers: the warpers exist only when it samples)
        if num_beams > 1 and warpers is not None:
            raise NotImplementedError("min_p / typical_p / epsilon_cutoff / eta_cutoff are built for sampling one sequence per row, "
                                      "not for num_beams > 1 (beam-sample needs min_tokens_to_keep = #eos + 1, i.e. M / K, and joint draws)")
        if num_beams > 1 and lproc is not None:
            raise NotImplementedError("repetition_penalty / no_repeat_ngram_size / bad_words_ids / min_length / min_new_tokens are "
                                      "built for greedy and sampling, not for num_beams > 1 (transformers applies them to the "
                                      "beams' log-softmax scores)")
        constraint = kwargs.pop("prefix_allowed_tokens_fn", None)
        if constraint is not None:
            from .constraint import is_constraint
            if not is_constraint(constraint):
                raise NotImplementedError("prefix_allowed_tokens_fn has to be a TokenTrie (or TokenTrie.per_row(...)): an arbitrary "
                                          "Python callback cannot run inside the captured decode step, and there is no host fallback")
            if num_beams > 1:
                raise NotImplementedError("prefix_allowed_tokens_fn is built for greedy and sampling, not for num_beams > 1 "
                                          "(transformers applies it to the beams' log-softmax scores)")
            if inputs is not None and constraint.n_rows() is not None and constraint.n_rows() != inputs.shape[0]:
                raise ValueError(f"TokenTrie.per_row holds {constraint.n_rows()} tries, the batch {inputs.shape[0]} rows")
            table = constraint.compiled()
            if vocab is not None and (table.min_id() < 0 or table.max_id() >= vocab):
                raise ValueError(f"the TokenTrie holds ids outside [0, {vocab}) (from {table.min_id()} to {table.max_id()})")
        sampler = None
        if do_sample:       # HF: temperature defaults to 1.0, top_p to 1.0; draws keyed by (seed, row, step)
            t = 1.0 if temperature is None else float(temperature)
            if not t > 0:
                raise ValueError("`temperature` has to be a strictly positive float when do_sample=True")
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # follows torch.manual_seed
            k = 0 if top_k is None else int(top_k)
            if k < 0:
                raise ValueError("`top_k` has to be a non-negative integer (0 / None: no top-k filtering)")
            sampler = (t, 1.0 if top_p is None else float(top_p), int(seed), k)
        if num_beams < 1:
            raise ValueError("`num_beams` has to be an integer strictly greater than 0")
        beam_pad = pad_id                                      # (HF's beam fill value distinguishes None / 0 from an id)
        if pad_id is None:
            pad_id = eos[0] if eos else 0
        if inputs is None:
            raise ValueError("generate() needs input ids")
        if return_prefix:                      # every check before the device is touched
            if not return_dict:
                raise ValueError("generate(return_prefix=True) needs return_dict_in_generate=True: the handle is a field of the output")
            for on, what in ((num_beams > 1, "num_beams > 1 (the beams' cache rows are permuted hypotheses, not answers)"),
                             (nret > 1, "num_return_sequences > 1"), (guidance is not None, "guidance_scale"),
                             (bool(lookup_k), "prompt_lookup_num_tokens")):
                if on:
                    raise NotImplementedError(f"generate(return_prefix=True) is built for greedy search and sampling of one answer "
                                              f"per row, not for {what}")
        if lookup_k:                           # every check before the device is touched
            lookup_m = _check_lookup(lookup_k, lookup_m, int(inputs.shape[0]), self.cfg.max_batch, do_sample=do_sample,
                                     num_beams=num_beams, nret=nret, guidance=guidance, prefix=prefix, lproc=lproc,
                                     constraint=constraint, outputs=return_dict and (bool(top_lp) or any(
                                         want[k] for k in ("output_scores", "output_logits", "output_token_logprobs"))))
            lookup_hist = lookup_history(inputs, attention_mask, lookup_ids, self.cfg.n_prot_tokens)
        if guidance is not None:               # every check before the device is touched
            if num_beams > 1:
                raise NotImplementedError("guidance_scale is built for greedy search and sampling, not for num_beams > 1 "
                                          "(transformers applies it to the beams' log-softmax scores)")
            if nret > 1:
                raise NotImplementedError("guidance_scale with num_return_sequences > 1 is not built: the fanned-out prefill has no "
                                          "paired negative rows")
            if prefix is not None:
                raise NotImplementedError("guidance_scale with generate(prefix=...) is not built: a detached prefix holds no rows "
                                          "for the negative prompts")
            P = int(inputs.shape[0])
            if neg_ids is None:
                neg_ids, neg_mask = protein_free_twin(inputs, attention_mask)
            else:
                neg_ids, neg_mask = _explicit_negative_prompt(neg_ids, neg_mask, P)
            max_len = int(getattr(getattr(self, "config", None), "tokenizer_model_max_length", None) or 0)
            T_pad = max(spliced_length(inputs, attention_mask, self.cfg.n_prot_tokens, max_len),
                        spliced_length(neg_ids, neg_mask, self.cfg.n_prot_tokens, max_len))
            if 2 * P > self.cfg.max_batch:
                raise _cabi.OpusError(-2, f"guidance_scale runs 2 x batch = 2 x {P} decoder rows: the context holds "
                                          f"max_batch={self.cfg.max_batch}")
            if T_pad > self.cfg.max_prompt:
                raise _cabi.OpusError(-2, f"guidance_scale pads the prompts and the negative prompts to {T_pad} positions: the "
                                          f"context holds max_prompt={self.cfg.max_prompt}")
        if prefix is not None:
            if num_beams > 1:
                raise NotImplementedError("generate(prefix=...) is built for greedy search and sampling, not for num_beams > 1")
            if nret > 1 and constraint is not None and constraint.n_rows() is not None:
                raise NotImplementedError("generate(prefix=..., num_return_sequences > 1) takes one TokenTrie for all rows, not "
                                          "TokenTrie.per_row: the rows are expanded on the host")
            embeds, behind = self._suffix_behind(prefix, prefix_rows, inputs, attention_mask, seq, seq_embedding, protein_tokens, nret)
            if lproc is not None:              # min_length counts the whole prompt: the prefix's slots and the spliced suffix
                pen, ngram, min_new, min_len, bad = lproc
                if min_new is None:
                    min_new = max((min_len or 0) - behind.Tp - int(embeds.shape[1]), 0)
                lproc = (pen, ngram, min_new, bad)
            self._set_logits_processors(lproc)
            self._set_token_constraint(constraint)
            self._set_warpers(warpers)
            outs = (want["output_token_logprobs"], want["output_scores"], want["output_logits"], top_lp) if return_dict else None
            res = self._greedy(embeds, None, max_new, eos, int(pad_id), sampler, outputs=outs, behind=behind)
            if return_prefix:                  # right behind the loop: nothing else has touched the context
                res.prefix = self._export_answer(res.sequences, eos, behind.new_kstart, behind.Tp + int(embeds.shape[1]))
            return res
        if num_beams <= 1 and nret > 1 and inputs.shape[0] * nret > self.cfg.max_batch:
            raise _cabi.OpusError(-2, f"num_return_sequences runs batch x num_return_sequences = {inputs.shape[0]} x {nret} decoder "
                                      f"rows: the context holds max_batch={self.cfg.max_batch}")
        if seq is not None:
            _, _, mask, _, embeds, _ = self.prepare_inputs_labels_for_multimodal(
                inputs, None, attention_mask if attention_mask is not None else torch.ones_like(inputs, dtype=torch.bool),
                None, None, seq, seq_embedding, inference_mode=True, protein_tokens=protein_tokens)
        else:
            dummy = torch.zeros((inputs.shape[0], self.cfg.n_prot_tokens, self.cfg.dec_dim), dtype=_cabi.operand_dtype(),
                                device=self.device)
            embeds, mask, _ = self._splice(inputs, attention_mask, dummy, True)
        if lproc is not None:                  # min_length counts the spliced prompt (transformers' _prepare_generated_length)
            pen, ngram, min_new, min_len, bad = lproc
            if min_new is None:
                min_new = max((min_len or 0) - int(embeds.shape[1]), 0)
            lproc = (pen, ngram, min_new, bad)
        if guidance is not None:               # the negative rows through the text-only splice, both sets to one length
            dummy = torch.zeros((neg_ids.shape[0], self.cfg.n_prot_tokens, self.cfg.dec_dim), dtype=_cabi.operand_dtype(),
                                device=self.device)
            n_embeds, n_mask, _ = self._splice(neg_ids, neg_mask, dummy, True)
            with torch.cuda.stream(self._stream):
                embeds, mask = pad_left_common(embeds, mask.to(torch.uint8), n_embeds, n_mask)
        self._set_logits_processors(lproc)
        self._set_token_constraint(constraint)
        self._set_warpers(warpers)
        if lookup_k:
            ids, stats = self._lookup(embeds, mask, max_new, eos, int(pad_id), lookup_k, lookup_m, lookup_hist)
            if not return_dict:
                return ids
            res = GenerateDecoderOnlyOutput(sequences=ids)
            res.stats = stats
            return res
        if guidance is not None:
            outs = (want["output_token_logprobs"], want["output_scores"], want["output_logits"], top_lp) if return_dict else None
            return self._greedy(embeds, mask, max_new, eos, int(pad_id), sampler, outputs=outs, guidance=guidance)
        if num_beams > 1:
            ids = self._beam_search(embeds, mask, max_new, eos, beam_pad, num_beams, sampler, nret)
            if not return_dict:
                return ids
            return GenerateBeamDecoderOnlyOutput(sequences=ids, sequences_scores=self.last_beam_scores.to(self.device))
        if not return_dict:
            return self._greedy(embeds, mask, max_new, eos, int(pad_id), sampler, nret=nret)
        res = self._greedy(embeds, mask, max_new, eos, int(pad_id), sampler,
                           outputs=(want["output_token_logprobs"], want["output_scores"], want["output_logits"], top_lp), nret=nret)
        if return_prefix:                      # right behind the loop: nothing else has touched the context
            first = mask.to(torch.int32).argmax(dim=1).cpu().numpy()      # (a row's first real slot: its kstart)
            res.prefix = self._export_answer(res.sequences, eos, first, int(embeds.shape[1]))
        return res

    def compute_transition_scores(self, sequences: torch.Tensor, scores, beam_indices: Optional[torch.Tensor] = None,
                                  normalize_logits: bool = False) -> torch.Tensor:
        """transformers' GenerationMixin.compute_transition_scores: the score of each generated token, [B, n].  `sequences`
        holds the new ids only (what generate() returns here); `scores` is out.scores or out.logits; normalize_logits=True
        applies a log-softmax over the vocabulary first (on out.logits: the token log-probabilities)."""
        V = scores[0].shape[-1]
        if beam_indices is None:
            beam_indices = torch.arange(scores[0].shape[0]).view(-1, 1).to(sequences.device)
            beam_indices = beam_indices.expand(-1, len(scores))
        stacked = torch.stack(scores).reshape(len(scores), -1).transpose(0, 1)
        if normalize_logits:
            stacked = torch.nn.functional.log_softmax(stacked.reshape(-1, V, stacked.shape[-1]), dim=1)
            stacked = stacked.reshape(-1, stacked.shape[-1])
        beam_mask = beam_indices < 0
        max_len = (1 - beam_mask.long()).sum(-1).max()
        beam_indices = beam_indices.clone()[:, :max_len]
        beam_mask = beam_mask[:, :max_len]
        beam_indices[beam_mask] = 0
        indices = sequences[:, sequences.shape[-1] - max_len:] + beam_indices * V
        out = stacked.gather(0, indices)
        out[beam_mask] = 0
        return out

    # TopKLogitsWarper of the sampling paths.  The reference pins transformers 4.46.3 (requirements.txt:20), whose
    # GenerationConfig.top_k defaults to 50 whenever it samples (transformers >= 5 defaults to None); the reference's drivers never
    # set it (run_opus_ddp.py:126-132), so 50 is what its sampling runs with.  generate(top_k=...) overrides per call; 0 / None = off.
    default_top_k = 50

    # Beam-sample: the reference's pin, transformers 4.46.3, sorts the M sampled continuations of a row by score (descending)
    # before its beam scorer looks at them, so "the first K may finish" means the K best of the draws; transformers >= 4.50
    # (`_get_top_k_continuations`, the installed 5.15 the host tests compare with) keeps the order drawn.  True = the pin.
    beam_sample_sorted = True

    def _set_top_k(self, k: int) -> None:
        if k != getattr(self, "_top_k", 0):
            _cabi.check(self._lib.opus_set_sampling_top_k(self._ctx, int(k)))
            self._top_k = int(k)

    def _beam_search(self, embeds, mask, max_new, eos, pad_id, K, sampler=None, nret: int = 1) -> torch.Tensor:
        """transformers GenerationMixin._beam_search (what run_opus_ddp.py:129,158 reaches with --num_beams K): B x K decoder rows,
        per step the device picks the M continuations of every batch row out of the K V - the best M by accumulated log-probability
        (opus_beam_topk; temperature 0) or, with `sampler` (temperature > 0: beam-sample), M drawn without replacement after the
        warpers (opus_beam_sample_topk) - and permutes the KV cache rows of the surviving beams (opus_kv_reorder); the host keeps
        the O(K) bookkeeping (beam.BeamState).  Returns the nret best finished sequences of every row [B nret, n], best first (rows
        that stopped earlier are filled as HF fills them); last_beam_scores [B nret]."""
        from .beam import BeamState
        B, T, _ = embeds.shape
        cfg = self.cfg
        if B * K > cfg.max_batch:
            raise _cabi.OpusError(-2, f"beam search runs batch x num_beams = {B} x {K} decoder rows: the context holds max_batch={cfg.max_batch}")
        if max_new > cfg.max_new_tokens:
            raise _cabi.OpusError(-2, f"max_new_tokens={max_new} exceeds the context's {cfg.max_new_tokens}")
        state = BeamState(B, K, max_new, eos, pad_id, cfg.dec_vocab)
        M = state.M
        if M > 16:
            raise NotImplementedError(f"beam search keeps max(2, 1 + #eos) x num_beams = {M} candidates per row; at most 16 are built")
        emb = embeds.repeat_interleave(K, dim=0).contiguous()          # _expand_inputs_for_generation: row b K + k
        msk = mask.repeat_interleave(K, dim=0).contiguous()
        self.prefill_logits(emb, msk)                                   # (the logits stay in the context)
        s = self._enter()
        with torch.cuda.stream(self._stream):
            d_run = torch.empty((B * K,), dtype=torch.float32, device=self.device)
            d_sc = torch.empty((B, M), dtype=torch.float32, device=self.device)
            d_ix = torch.empty((B, M), dtype=torch.int32, device=self.device)
            ident = np.tile(np.arange(K, dtype=np.int64), (B, 1))
            base = (np.arange(B, dtype=np.int64) * K)[:, None]
            if sampler is not None:
                self._set_top_k(sampler[3] if len(sampler) > 3 else self.default_top_k)
            while True:
                d_run.copy_(torch.from_numpy(state.running_scores.reshape(-1)), non_blocking=True)
                if sampler is None:
                    _cabi.check(self._lib.opus_beam_topk(self._ctx, d_run.data_ptr(), B, K, M, d_sc.data_ptr(), d_ix.data_ptr(), s))
                else:
                    _cabi.check(self._lib.opus_beam_sample_topk(self._ctx, None, d_run.data_ptr(), B, K, M, sampler[0], sampler[1],
                                                                sampler[2], state.cur, d_sc.data_ptr(), d_ix.data_ptr(), s))
                sc, ix = d_sc.cpu().numpy(), d_ix.cpu().numpy()         # (synchronises this stream)
                # (fp32 softmax gives exactly zero below exp(-103.97): continuations that far under the row's best - filtered ones,
                #  those of dead beams at -1e9 - are the "non-negative categories" torch.multinomial finds too few of)
                if sampler is not None and ((ix == 0x7fffffff) | (sc < sc.max(axis=1, keepdims=True) - 103.0)).any():
                    self._leave()
                    raise RuntimeError("invalid multinomial distribution (with replacement=False, not enough non-negative category "
                                       f"to sample): beam-sample draws {M} continuations per row, the temperature / top_k / top_p "
                                       "filters left fewer")        # (torch.multinomial's message: what the reference raises here)
                if sampler is not None and self.beam_sample_sorted:     # 4.46.3: torch.sort(next_token_scores, descending=True) behind the draw
                    order = np.argsort(-sc, axis=1, kind="stable")
                    sc, ix = np.take_along_axis(sc, order, 1), np.take_along_axis(ix, order, 1)
                tok, src, done = state.step(sc, ix)
                if done:
                    break
                if not np.array_equal(src, ident):
                    d_src = torch.from_numpy((src + base).reshape(-1).astype(np.int32)).to(self.device)
                    _cabi.check(self._lib.opus_kv_reorder(self._ctx, d_src.data_ptr(), B * K, s))
                d_tok = torch.from_numpy(tok.reshape(-1).astype(np.int32)).to(self.device)
                _cabi.check(self._lib.opus_llama_decode_step(self._ctx, d_tok.data_ptr(), None, s))
        self._leave()
        self.last_beam_scores = torch.from_numpy(state.result_scores(nret))
        return torch.from_numpy(state.result(nret)).to(self.device)

    def set_stop_sequence(self, ids: Optional[Sequence[int]]) -> None:
        """Opt-in early stop: a row is finished once its new ids end with `ids` (at most 8) - e.g.
        tokenizer.encode("###", add_special_tokens=False), the marker the reference cuts the decoded text at
        (eval/run_opus_ddp.py:19-27).  The cut text is unchanged; a batch whose rows have all stopped ends early.
        None / empty clears it (the reference's behaviour: decode to max_new_tokens)."""
        ids = [int(t) for t in ids] if ids is not None else []
        if ids == getattr(self, "_stop_ids", []):
            return
        arr = (C.c_int32 * max(1, len(ids)))(*ids)
        _cabi.check(self._lib.opus_set_stop_sequence(self._ctx, arr, len(ids)))
        self._stop_ids = ids

    def _set_warpers(self, setting) -> None:
        """setting = (min_p, typical_p, epsilon_cutoff, eta_cutoff) or None (off: 0, 1, 0, 0), applied to this context's following
        sampling calls; an unchanged setting costs nothing.  The captured decode step reads the values from device memory."""
        setting = tuple(float(x) for x in setting) if setting is not None else _WARPERS_OFF
        if setting != getattr(self, "_warpers", _WARPERS_OFF):
            _cabi.check(self._lib.opus_set_sampling_warpers(self._ctx, *setting))
            self._warpers = setting

    def _set_logits_processors(self, setting) -> None:
        """setting = (repetition_penalty, no_repeat_ngram_size, min_new_tokens, bad_words_ids tuple) or None (off), applied to
        this context's following generate calls; an unchanged setting costs nothing."""
        if setting is not None and setting == (1.0, 0, 0, ()):
            setting = None
        if setting == getattr(self, "_lproc", None):
            return
        if setting is None:
            _cabi.check(self._lib.opus_set_logits_processors(self._ctx, 1.0, 0, 0, None, None, 0))
        else:
            pen, ngram, min_new, bad = setting
            flat = [t for w in bad for t in w]
            offs = np.cumsum([0] + [len(w) for w in bad]).tolist()
            ids = (C.c_int32 * max(1, len(flat)))(*flat)
            off = (C.c_int32 * len(offs))(*offs)
            _cabi.check(self._lib.opus_set_logits_processors(self._ctx, float(pen), int(ngram), int(min_new), ids, off, len(bad)))
        self._lproc = setting

    def _set_token_constraint(self, constraint) -> None:
        """constraint: a TokenTrie / TokenTrie.per_row object or None (off), applied to this context's following generate calls.
        The table is uploaded only when the object differs from the one this context holds; None when none is held costs nothing."""
        if constraint is getattr(self, "_constraint", None):
            return
        s = self._enter()
        try:
            if constraint is None:
                _cabi.check(self._lib.opus_set_token_constraint(self._ctx, 0, None, None, None, 0, None, None, 0, None, 0, s))
            else:
                t = constraint.compiled()
                p = lambda a: a.ctypes.data if a.size else None                              # noqa: E731
                _cabi.check(self._lib.opus_set_token_constraint(self._ctx, t.n_states, p(t.edge_off), p(t.edge_tok), p(t.edge_next),
                                                                t.n_edges, p(t.completing), p(t.end_ids), len(t.end_ids),
                                                                p(t.start), len(t.start), s))
        finally:
            self._leave()
        self._constraint = constraint

    def _greedy(self, embeds, mask, max_new, eos, pad_id, sampler=None, outputs=None, nret: int = 1, behind=None,
                guidance: Optional[float] = None):
        """outputs = (token_logprobs, scores, logits) flags (+ top_logprobs' k, 0 = off): a GenerateDecoderOnlyOutput instead of the ids.
        nret > 1: the B prompts are prefilled once and decoded as B nret rows (opus_generate_scored_fanout); every result has
        B nret rows.
        behind (a _BehindCall; mask unused, nret 1): embeds are right-padded suffix rows behind a detached prefix
        (opus_generate_scored_behind).
        guidance (nret 1, no behind): embeds / mask hold P conditional rows, then their P negative rows
        (opus_generate_scored_guided); every result has P rows."""
        P, T, _ = embeds.shape                           # P prompts, B decoder rows
        B = P * nret
        if guidance is not None:
            P = B = P // 2                               # (rows with ids and outputs: the conditional half)
        V = self.cfg.dec_vocab
        embeds = embeds.contiguous()
        if behind is None:
            mask = mask.to(torch.uint8).contiguous()
        s = self._enter()
        with torch.cuda.stream(self._stream):
            # one persistent id buffer: its address is part of the captured decode graph's identity
            if getattr(self, "_out_ids", None) is None or self._out_ids.shape[0] < B or self._out_ids.shape[1] < max_new:
                self._out_ids = torch.empty((max(B, self.cfg.max_batch), max(max_new, self.cfg.max_new_tokens)),
                                            dtype=torch.int32, device=self.device)
            out = self._out_ids.view(-1)[: B * max_new].view(B, max_new)
            out.fill_(pad_id)
            n_out = C.c_int32(0)
            eos_arr = (C.c_int32 * max(1, len(eos)))(*eos)
            if sampler is not None:
                self._set_top_k(sampler[3] if len(sampler) > 3 else self.default_top_k)
            lp = sc = lg = None
            top_k = 0
            if outputs is not None:
                want_lp, want_sc, want_lg = outputs[:3]
                top_k = int(outputs[3]) if len(outputs) > 3 else 0
                # fresh caller-owned tensors every call: their addresses reach the captured step through a device descriptor
                lp = torch.zeros((B, max_new), dtype=torch.float32, device=self.device) if want_lp else None
                sc = torch.empty((max_new, B, V), dtype=torch.float32, device=self.device) if want_sc else None
                lg = torch.empty((max_new, B, V), dtype=torch.float32, device=self.device) if want_lg else None
                if (sampler is None and sc is not None and lg is not None and getattr(self, "_lproc", None) is None
                        and getattr(self, "_constraint", None) is None and guidance is None):
                    lg = None                                   # greedy: the processed scores are the logits - one tensor
            # one entry per prefill; with no output pointers each is the plain call (the same launches and graph)
            if guidance is not None:
                entry, head = self._lib.opus_generate_scored_guided, (embeds.data_ptr(), mask.data_ptr(), P, T, guidance)
            elif behind is not None:
                entry, head = self._lib.opus_generate_scored_behind, (behind.snap, embeds.data_ptr(), B, T, behind.lens, behind.src)
            elif nret > 1:                               # (sampling: greedy search takes no num_return_sequences)
                entry, head = self._lib.opus_generate_scored_fanout, (embeds.data_ptr(), mask.data_ptr(), P, T, nret)
            else:
                entry, head = self._lib.opus_generate_scored, (embeds.data_ptr(), mask.data_ptr(), B, T)
            t, p, sd = (sampler[0], sampler[1], sampler[2]) if sampler is not None else (0.0, 1.0, 0)
            ptr = lambda x: None if x is None else x.data_ptr()                              # noqa: E731
            if top_k:                                    # (steps the loop never ran keep the finished row's values)
                top_ids = torch.full((B, max_new, top_k), -1, dtype=torch.int32, device=self.device)
                top_val = torch.zeros((B, max_new, top_k), dtype=torch.float32, device=self.device)
                _cabi.check(self._lib.opus_set_gen_top_logprobs(self._ctx, top_k, top_ids.data_ptr(), top_val.data_ptr()))
            try:
                _cabi.check(entry(self._ctx, *head, max_new, eos_arr, len(eos), pad_id, t, p, sd, out.data_ptr(), C.byref(n_out),
                                  ptr(lp), ptr(sc), ptr(lg), s))
            finally:
                if top_k:
                    self._lib.opus_set_gen_top_logprobs(self._ctx, 0, None, None)
        self._leave()
        n = n_out.value
        ids = out[:, :n].long()                          # (a copy: the id buffer is reused by the next call)
        if outputs is None:
            return ids
        res = GenerateDecoderOnlyOutput(sequences=ids)
        if want_sc:
            res.scores = tuple(sc[k] for k in range(n))
        if want_lg:
            res.logits = res.scores if lg is None else tuple(lg[k] for k in range(n))
        if want_lp:
            res.token_logprobs = lp[:, :n]
            res.logprob = res.token_logprobs.sum(dim=1)
            res.n_tokens = counted_tokens(ids, eos, getattr(self, "_stop_ids", []))
        if top_k:
            res.top_logprobs = top_val[:, :n]
            res.top_ids = top_ids[:, :n].long()
        return res

    # ------------------------------------------------------------------ prompt-lookup decoding
    def _lookup(self, embeds, mask, max_new, eos, pad_id, k: int, max_ngram: int, hist):
        """generate(prompt_lookup_num_tokens=k) behind the splice: opus_generate_lookup on the rows' histories (lookup_history).
        Returns (new ids [B, n], LookupStats)."""
        B, T, _ = embeds.shape
        embeds = embeds.contiguous()
        mask = mask.to(torch.uint8).contiguous()
        rows, lens = hist
        s = self._enter()
        with torch.cuda.stream(self._stream):
            if getattr(self, "_out_ids", None) is None or self._out_ids.shape[0] < B or self._out_ids.shape[1] < max_new:
                self._out_ids = torch.empty((max(B, self.cfg.max_batch), max(max_new, self.cfg.max_new_tokens)),
                                            dtype=torch.int32, device=self.device)
            out = self._out_ids.view(-1)[: B * max_new].view(B, max_new)
            out.fill_(pad_id)
            d_hist = torch.from_numpy(rows).to(self.device)
            n_out = C.c_int32(0)
            eos_arr = (C.c_int32 * max(1, len(eos)))(*eos)
            len_arr = (C.c_int32 * B)(*[int(v) for v in lens])
            stats = (C.c_int64 * 4)()
            _cabi.check(self._lib.opus_generate_lookup(self._ctx, embeds.data_ptr(), mask.data_ptr(), B, T, max_new, eos_arr, len(eos),
                                                       pad_id, k, max_ngram, d_hist.data_ptr(), rows.shape[1], len_arr,
                                                       out.data_ptr(), C.byref(n_out), stats, s))
        self._leave()
        return out[:, :n_out.value].long(), LookupStats(*[int(v) for v in stats])

    def verify_step(self, tokens: torch.Tensor, draft_len: Optional[torch.Tensor] = None, return_logits: bool = True):
        """One verify pass on the current decode state (behind prefill_logits() / decode_logits() / an earlier verify_step):
        tokens int [R, n] - column 0 the token whose K / V are not cached yet, then a draft of draft_len[r] ids (None: n - 1).
        Returns (logits fp32 [R, n, V] or None, argmax int32 [R, n], a): position j holds the model's prediction behind
        tokens[:, : j + 1]; a is the lockstep acceptance (the shortest accepted draft prefix over the rows), and the decode
        state has advanced by a + 1 positions.  R n <= max_batch."""
        tokens = tokens.to(self.device, torch.int32).contiguous()
        R, n = tokens.shape
        if draft_len is not None:
            draft_len = draft_len.to(self.device, torch.int32).contiguous()
        s = self._enter()
        with torch.cuda.stream(self._stream):
            logits = torch.empty((R, n, self.cfg.dec_vocab), dtype=torch.float32, device=self.device) if return_logits else None
            arg = torch.empty((R, n), dtype=torch.int32, device=self.device)
            a = C.c_int32(0)
            _cabi.check(self._lib.opus_llama_verify_step(self._ctx, tokens.data_ptr(), n,
                                                         None if draft_len is None else draft_len.data_ptr(),
                                                         None if logits is None else logits.data_ptr(), arg.data_ptr(),
                                                         C.byref(a), s))
        self._leave()
        return logits, arg, a.value

    # ------------------------------------------------------------------ continuous batching
    _CONTINUOUS_UNSUPPORTED = ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask", "prefix", "prefix_rows",
                               "prefix_allowed_tokens_fn", "repetition_penalty", "no_repeat_ngram_size", "bad_words_ids",
                               "min_length", "min_new_tokens", "output_scores", "output_logits", "output_token_logprobs",
                               "top_logprobs")

    @torch.no_grad()
    def generate_continuous(self, prompts, seqs=None, max_new_tokens: int = 32, eos_token_id=None, pad_token_id=None,
                            slots: Optional[int] = None, refill_min: Optional[int] = None, do_sample: bool = False,
                            temperature=None, top_p=None, top_k="default", seed=None, stop_sequence=None, seq_embedding=None,
                            protein_tokens=None, return_dict_in_generate: bool = False, **kwargs):
        """Answers N prompts through ONE decode batch of `slots` rows that is kept full: a row whose answer has ended (an EOS id,
        the stop sequence, max_new_tokens ids) is handed to the next queued prompt while the other rows keep decoding, instead of
        decoding pad ids until the batch's longest answer ends as generate() does.

        prompts: N 1-D id tensors, unpadded, <seq> placeholders as in generate(); `seqs` / `seq_embedding` / `protein_tokens`
        carry N entries (one protein per prompt).  Returns a list of N 1-D int64 tensors in input order: each prompt's new ids up
        to and including its EOS id or the last id of the stop sequence, at most max_new_tokens - what generate() returns for that
        row, without the pad tail.  return_dict_in_generate=True: an object with `sequences` (that list), `n_tokens` int64 [N]
        and `stats`, a dict of sessions, decode_steps, refills, rows_refilled, live_row_steps, slot_steps (occupancy =
        live_row_steps / slot_steps).

        slots (default and at most cfg.max_batch): decode rows.  refill_min (default max(1, slots // 4)): rows that must be free
        before a refill is worth its prefill; ignored when the queue could otherwise not progress.  The context's
        max_new_tokens capacity S is a session's step budget: a row can only begin at a step t with t + max_new_tokens <= S, so
        create the context with a few times the token budget (continuous.py holds the schedule).  New prompts are prefilled in
        a helper context (new_context(), created on first use and kept) and their K / V placed under the free rows.

        Greedy and sampling (with generate()'s min_p / typical_p / epsilon_cutoff / eta_cutoff), EOS ids and the stop sequence.  Draws are keyed by (seed, decode row, session step), so the same
        call twice gives the same ids, but a sampled run is NOT the generate() run of the same seed (a prompt's row and step
        differ).  Greedy ids are generate()'s wherever the top-1 margin is decisive: a refilled row's K / V come from the same
        prefill kernels, at other cache slots.  num_beams > 1, num_return_sequences > 1, guidance_scale, prefix=,
        prefix_allowed_tokens_fn, the logits processors and output_scores / output_logits / output_token_logprobs raise
        NotImplementedError; a capacity violation raises OpusError -2."""
        from . import continuous as cont
        for k in self._CONTINUOUS_UNSUPPORTED:
            v = kwargs.pop(k, None)
            if v is not None and v is not False and not (k == "repetition_penalty" and float(v) == 1.0) \
                    and not (k in ("no_repeat_ngram_size", "min_length", "min_new_tokens") and int(v) == 0) \
                    and not (k == "guidance_scale" and float(v) == 1.0):
                raise NotImplementedError(f"generate_continuous({k}=...) is not built: {k} counts a row's steps from the start of "
                                          "the decode batch, and a refilled row begins later")
        for k in ("num_beams", "num_return_sequences"):
            v = kwargs.pop(k, None)
            if v is not None and int(v) > 1:
                raise NotImplementedError(f"generate_continuous({k}={int(v)}) is not built: one decode row per prompt")
        for k in ("use_cache", "position_ids", "attention_mask"):
            kwargs.pop(k, None)
        warpers = _sampling_warpers(kwargs)
        if not do_sample:
            warpers = None
        if kwargs:
            raise TypeError(f"generate_continuous() got unexpected arguments {sorted(kwargs)}")
        if prompts is None or len(prompts) == 0:
            raise ValueError("generate_continuous() needs a list of prompts")
        prompts = [torch.as_tensor(p).detach().to("cpu", torch.int64).reshape(-1) for p in prompts]
        N = len(prompts)
        for name, x in (("seqs", seqs), ("seq_embedding", seq_embedding), ("protein_tokens", protein_tokens)):
            if x is not None and len(x) != N:
                raise ValueError(f"`{name}` carries {len(x)} entries for {N} prompts")
        cfg = self.cfg
        max_new = int(max_new_tokens)
        slots = cfg.max_batch if slots is None else int(slots)
        max_len = int(getattr(getattr(self, "config", None), "tokenizer_model_max_length", None) or 0)
        lens = [spliced_length(p[None], None, cfg.n_prot_tokens, max_len) for p in prompts]
        bad = cont.check_capacity(lens, slots, max_new, cfg.max_new_tokens, cfg.max_prompt, cfg.max_batch)
        if bad:
            raise _cabi.OpusError(-2, "generate_continuous: " + bad)
        g = self.generation_config
        eos = g.eos_token_id if eos_token_id is None else eos_token_id
        eos = [] if eos is None else ([int(eos)] if isinstance(eos, int) else [int(e) for e in eos])
        pad_id = g.pad_token_id if pad_token_id is None else pad_token_id
        pad_id = int(pad_id) if pad_id is not None else (eos[0] if eos else 0)
        sampler = None
        if do_sample:
            t = 1.0 if temperature is None else float(temperature)
            if not t > 0:
                raise ValueError("`temperature` has to be a strictly positive float when do_sample=True")
            k = self.default_top_k if isinstance(top_k, str) else (0 if top_k is None else int(top_k))
            if k < 0:
                raise ValueError("`top_k` has to be a non-negative integer (0 / None: no top-k filtering)")
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            sampler = (t, 1.0 if top_p is None else float(top_p), int(seed), k)
        # ---- the device from here on
        if self._lib.opus_stream_lag() != cont.LAG:
            raise _cabi.OpusError(-101, "opus_stream_lag() differs from continuous.LAG")
        self.set_stop_sequence(stop_sequence)
        self._set_logits_processors(None)
        self._set_token_constraint(None)
        self._set_warpers(warpers)
        if sampler is not None:
            self._set_top_k(sampler[3])
        backend = _StreamBackend(self, prompts, lens, seqs, seq_embedding, protein_tokens, max_new, eos, pad_id, sampler, slots)
        stats = cont.run_schedule(lens, slots, max_new, cfg.max_new_tokens, refill_min, backend)
        stats.pop("placements", None)
        out = backend.results()
        if not return_dict_in_generate:
            return out
        return ContinuousOutput(sequences=out, n_tokens=torch.tensor([int(x.numel()) for x in out], dtype=torch.int64), stats=stats)

    def generate_from_tokens(self, d_tokens, d_lens, input_ids: torch.Tensor,
                             attention_mask: Optional[torch.Tensor], max_new_tokens: int, eos: Sequence[int] = (),
                             pad_token_id: int = 0, bucket_rows: Optional[Sequence[torch.Tensor]] = None,
                             sampler=None) -> torch.Tensor:
        """generate() for callers whose inputs are already resident in HBM: ESM-2 token ids int32
        [B,T] + lens int32 [B] (alphabet.batch_convert), prompt ids int64 [B,T_text] on the device.
        Same result as generate(input_ids, seqs, ...); used by bench.py for the timed region.
        Length-bucketed form: d_tokens / d_lens / bucket_rows are lists (one entry per bucket; bucket_rows[k] =
        int64 device tensor with the batch rows of bucket k), as encode_seq2embedding buckets strings."""
        cfg = self.cfg
        B = input_ids.shape[0]
        self._set_logits_processors(None)       # (a previous generate()'s processors do not carry over; no-op when off)
        self._set_token_constraint(None)
        self._set_warpers(None)
        if bucket_rows == "packed":      # d_tokens: packed int32 [M] on the device; d_lens: the HOST row offsets cu [B + 1]
            s = self._enter()
            with torch.cuda.stream(self._stream):
                pooled = torch.empty((B, cfg.enc_dim), dtype=torch.float32, device=self.device)
                cu_arr = (C.c_int32 * (B + 1))(*[int(v) for v in d_lens])
                _cabi.check(self._lib.opus_esm2_encode_packed(self._ctx, d_tokens.data_ptr(), cu_arr, B, pooled.data_ptr(), s))
                prot = torch.empty((B, cfg.n_prot_tokens, cfg.dec_dim), dtype=_cabi.operand_dtype(), device=self.device)
                _cabi.check(self._lib.opus_projector_forward(self._ctx, pooled.data_ptr(), B, prot.data_ptr(), None, s))
            self._leave()
            emb, mask, _ = self._splice(input_ids, attention_mask, prot, True)
            return self._greedy(emb, mask, int(max_new_tokens), [int(e) for e in eos], int(pad_token_id), sampler)
        buckets = list(zip(d_tokens, d_lens, bucket_rows)) if bucket_rows is not None else [(d_tokens, d_lens, None)]
        s = self._enter()
        with torch.cuda.stream(self._stream):
            pooled = torch.empty((B, cfg.enc_dim), dtype=torch.float32, device=self.device)
            for tok, lens, rows in buckets:
                out = pooled if rows is None else torch.empty((tok.shape[0], cfg.enc_dim), dtype=torch.float32, device=self.device)
                _cabi.check(self._lib.opus_esm2_encode(self._ctx, tok.data_ptr(), lens.data_ptr(), tok.shape[0], tok.shape[1],
                                                       out.data_ptr(), s))
                if rows is not None:
                    pooled[rows] = out
            prot = torch.empty((B, cfg.n_prot_tokens, cfg.dec_dim), dtype=_cabi.operand_dtype(), device=self.device)
            _cabi.check(self._lib.opus_projector_forward(self._ctx, pooled.data_ptr(), B, prot.data_ptr(), None, s))
        self._leave()
        emb, mask, _ = self._splice(input_ids, attention_mask, prot, True)
        return self._greedy(emb, mask, int(max_new_tokens), [int(e) for e in eos], int(pad_token_id), sampler)

    # ------------------------------------------------------------------ teacher-forced scoring
    @torch.no_grad()
    def forward(self, input_ids: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.Tensor] = None, past_key_values=None, labels: Optional[torch.Tensor] = None,
                use_cache: Optional[bool] = None, output_attentions: Optional[bool] = None,
                output_hidden_states: Optional[bool] = None, seq=None, input_embed: Optional[torch.Tensor] = None,
                return_dict: Optional[bool] = None, protein_tokens: Optional[torch.Tensor] = None, return_logits: bool = True,
                top_logprobs: Optional[int] = None, **kwargs):
        """opus_llama.py:41-92 (+ LlamaForCausalLM.forward): with `seq` (or `input_embed` pooled embeddings / `protein_tokens`
        projected blocks) the proteins are spliced into the prompt in training mode (right padding, IGNORE_INDEX labels on the
        protein slots); otherwise `input_ids` are embedded (or `inputs_embeds` taken as they are).  Returns a CausalLMOutput:
        `loss` = HF's causal-LM loss (target of position t is labels[b, t + 1]; -100 ignored; fp32 mean over the counted targets,
        NaN when none is counted), `logits` [B, T, V] in the operand dtype (None with return_logits=False; values at masked
        positions are unspecified), `past_key_values` = None; extensions `token_logprobs` fp32 [B, T] (log p(labels[b, t]) at
        counted targets, 0 elsewhere) and `n_tokens`.  top_logprobs=k (an int in 1..20, with labels): `top_logprobs` fp32 / `top_ids`
        int64 [B, T, k], at every counted target labels[b, t] the k likeliest ids of the distribution that predicts it (value
        descending, then id ascending, on the 16-bit logits) and their log-probabilities; 0 / -1 elsewhere.  With
        return_logits=False it still runs the lm_head on all positions of a group of max_batch rows, into one group's buffer that is
        dropped at the end of the call: both values of return_logits then give identical lists and token_logprobs.
        Rows are right-padded or unpadded; left-padded rows only with position_ids == cumsum(mask) - 1 on their real slots (what
        the kernels compute; HF would use arange positions).  Overwrites this context's KV cache: decode_step fails until the next
        prefill / generate.  Batches above max_batch run in groups of max_batch rows (one loss over all of them)."""
        if past_key_values is not None:
            raise NotImplementedError("forward(): `past_key_values` input is not supported (no incremental scoring)")
        if use_cache:
            raise NotImplementedError("forward(): use_cache=True is not supported (no cache is returned)")
        if output_attentions or output_hidden_states:
            raise NotImplementedError("forward(): output_attentions / output_hidden_states are not supported")
        inputs_embeds = kwargs.pop("inputs_embeds", None)
        if kwargs:
            raise TypeError(f"forward() got unexpected keyword arguments {sorted(kwargs)}")
        cfg = self.cfg
        top_k = _top_logprobs_arg(top_logprobs, cfg.dec_vocab)
        if top_k and labels is None:
            raise ValueError("forward(top_logprobs=k) needs labels: the alternatives are those of the counted targets")
        embeds = None
        if seq is not None or input_embed is not None or protein_tokens is not None:
            if input_ids is None:
                raise ValueError("forward() with proteins needs input_ids (the prompt with its <seq> placeholders)")
            mask_in = attention_mask if attention_mask is not None else torch.ones_like(input_ids, dtype=torch.bool)
            _, _, mask, _, embeds, labels = self.prepare_inputs_labels_for_multimodal(
                input_ids, None, mask_in, None, labels, seq if seq is not None else (), input_embed, inference_mode=False,
                protein_tokens=protein_tokens)
            position_ids = None                                 # (the splice's rows are right-padded, positions 0..n-1)
        if embeds is None:
            if inputs_embeds is not None:
                if input_ids is not None:
                    raise ValueError("You cannot specify both input_ids and inputs_embeds at the same time")
                embeds = inputs_embeds
            else:
                if input_ids is None:
                    raise ValueError("You have to specify either input_ids or inputs_embeds")
                ids = input_ids.long()
                if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= cfg.dec_vocab):
                    raise ValueError(f"input_ids must lie in [0, {cfg.dec_vocab}) without proteins (a <seq> placeholder needs seq=)")
                embeds = self.model.embed_tokens(ids)
            mask = attention_mask
        if embeds.dim() != 3 or embeds.shape[2] != cfg.dec_dim:
            raise ValueError(f"embeddings must be [B, T, {cfg.dec_dim}], got {tuple(embeds.shape)}")
        B, T, _ = embeds.shape
        if T > cfg.max_prompt:
            raise _cabi.OpusError(-2, f"forward: T={T} positions exceed max_prompt={cfg.max_prompt}")
        m = np.ones((B, T), dtype=bool) if mask is None else mask.detach().cpu().bool().numpy()
        if m.shape != (B, T):
            raise ValueError(f"attention_mask {m.shape} does not match the embeddings' [B, T] = {(B, T)}")
        _check_forward_mask(m, None if position_ids is None else position_ids.detach().cpu().numpy())
        lab = None
        if labels is not None:
            lab = labels.detach().cpu().long().numpy()
            if lab.shape != (B, T):
                raise ValueError(f"labels {lab.shape} do not match the embeddings' [B, T] = {(B, T)}")
            bad = (lab != IGNORE_INDEX) & ((lab < 0) | (lab >= cfg.dec_vocab))
            if bad.any():
                raise ValueError(f"labels must be {IGNORE_INDEX} or lie in [0, {cfg.dec_vocab})")
            src = np.zeros((B, T), dtype=bool)
            src[:, :-1] = lab[:, 1:] != IGNORE_INDEX                # counted target of position t: labels[b, t + 1]
            if (src & ~m).any():
                b, t = map(int, np.argwhere(src & ~m)[0])
                raise ValueError(f"labels[{b}, {t + 1}] is counted but its source position {t} is masked out: "
                                 "its logits are not defined on this path")
        else:
            src = np.zeros((B, T), dtype=bool)

        dev, dt = self.device, _cabi.operand_dtype()
        embeds = embeds.to(dev, dt).contiguous()
        mask_u8 = torch.from_numpy(m.astype(np.uint8)).to(dev)
        token_lp = torch.zeros((B, T), dtype=torch.float32, device=dev)
        logits = torch.empty((B, T, cfg.dec_vocab), dtype=dt, device=dev) if return_logits else None
        top_val = torch.zeros((B, T, top_k), dtype=torch.float32, device=dev) if top_k else None
        top_ids = torch.full((B, T, top_k), -1, dtype=torch.int64, device=dev) if top_k else None
        G = cfg.max_batch
        # top log-probs without returned logits: the lm_head still runs on all rows of a group, as with return_logits=True, into
        # one group's buffer that lives for the call - the two paths then share their GEMM launches and give identical lists
        # (the loss-only lm_head runs at another row count through other kernels, whose 16-bit logits differ in the last bit)
        full = return_logits or bool(top_k)
        group_logits = torch.empty((min(B, G), T, cfg.dec_vocab), dtype=dt, device=dev) if full and not return_logits else None
        tgt_all = np.full((B, T), -1, dtype=np.int32)
        if lab is not None:
            tgt_all[:, :-1] = np.where(src[:, :-1], lab[:, 1:], -1)
        cc = _cabi.CConfig.from_config(cfg)
        R_max = min(B, G) * T if full else max(int(src[g0:g0 + G].sum()) for g0 in range(0, B, G))
        n_scratch = int(self._lib.opus_llama_forward_scratch_bytes(C.byref(cc), R_max, 1 if full else 0))
        s = self._enter()
        with torch.cuda.stream(self._stream):
            scratch = torch.empty((max(n_scratch, 1),), dtype=torch.uint8, device=dev)
            keep = []
            for g0 in range(0, B, G):
                Bg = min(G, B - g0)
                if full:
                    rows = np.arange(Bg * T, dtype=np.int32)
                    tg = tgt_all[g0:g0 + Bg].reshape(-1)
                else:
                    rows = np.flatnonzero(src[g0:g0 + Bg].reshape(-1)).astype(np.int32)
                    tg = tgt_all[g0:g0 + Bg].reshape(-1)[rows]
                R = int(rows.size)
                d_rows = torch.from_numpy(rows).to(dev, non_blocking=True) if R else None
                d_tg = torch.from_numpy(np.ascontiguousarray(tg)).to(dev, non_blocking=True) if R else None
                lp = torch.empty((max(R, 1),), dtype=torch.float32, device=dev)
                if top_k:                                               # [R, k] in the order of rows (opus_set_gen_top_logprobs)
                    r_ids = torch.full((max(R, 1), top_k), -1, dtype=torch.int32, device=dev)
                    r_val = torch.zeros((max(R, 1), top_k), dtype=torch.float32, device=dev)
                    _cabi.check(self._lib.opus_set_gen_top_logprobs(self._ctx, top_k, r_ids.data_ptr(), r_val.data_ptr()))
                try:
                    _cabi.check(self._lib.opus_llama_forward(
                        self._ctx, embeds[g0:].data_ptr(), mask_u8[g0:].data_ptr(), Bg, T,
                        None if d_rows is None else d_rows.data_ptr(), R, None if d_tg is None else d_tg.data_ptr(), lp.data_ptr(),
                        (logits[g0:] if return_logits else group_logits).data_ptr() if full else None, scratch.data_ptr(), n_scratch, s))
                finally:
                    if top_k:
                        self._lib.opus_set_gen_top_logprobs(self._ctx, 0, None, None)
                if top_k and R:                                         # position t predicts the label at t + 1
                    counted = torch.from_numpy(np.flatnonzero(src[g0:g0 + Bg].reshape(-1)).astype(np.int64)).to(dev)
                    top_val[g0:g0 + Bg].view(-1, top_k)[counted + 1] = r_val[counted]
                    top_ids[g0:g0 + Bg].view(-1, top_k)[counted + 1] = r_ids[counted].long()
                    keep.append((r_ids, r_val))
                if full:
                    token_lp[g0:g0 + Bg, 1:] = lp.view(Bg, T)[:, :-1]
                elif R:
                    flat = token_lp[g0:g0 + Bg].view(-1)                # position t scores the label at t + 1
                    flat[torch.from_numpy(rows.astype(np.int64) + 1).to(dev)] = lp[:R]
                keep.append((d_rows, d_tg, lp))
            n_tokens = int(src.sum())
            loss = None
            if lab is not None:
                loss = -token_lp.sum() / n_tokens if n_tokens else torch.tensor(float("nan"), device=dev)
        self._leave()
        out = CausalLMOutput(loss=loss, logits=logits, token_logprobs=token_lp, n_tokens=n_tokens)
        if top_k:
            out.top_logprobs, out.top_ids = top_val, top_ids
        if return_dict is False:
            return out.to_tuple()
        return out

    __call__ = forward

    # ------------------------------------------------------------------ shared-prefix scoring
    @torch.no_grad()
    def cache_prefix(self, input_ids: torch.Tensor, seq=None, attention_mask: Optional[torch.Tensor] = None,
                     seq_embedding=None, protein_tokens: Optional[torch.Tensor] = None, detach: bool = False,
                     last_logits: bool = False, prefix: Optional["OpusPrefix"] = None, prefix_rows=None) -> "OpusPrefix":
        """Prefills a prompt batch once and returns a handle that score_continuations() ranks continuations against.  The inputs
        are prepared exactly as generate() prepares them (inference-mode splice with `seq` / `seq_embedding` / `protein_tokens`;
        left-padded or unpadded rows): it IS a prefill, decode_logits() continues it as after prefill_logits().  The last slot of
        every row must be a real token (ValueError otherwise).  The handle is valid until the next call on this context that
        prefills or permutes the cache (cache_prefix, generate, forward, prefill_logits, beam search); decode steps keep it.
        prefix=OpusPrefix (+ prefix_rows, as in generate(prefix=...)): `input_ids` are SUFFIX rows behind that handle, teacher-
        forced without generating (opus_llama_prefix_behind: the handle's K / V placed, only the suffix prefilled).  The result is
        a LIVE handle on this context of prefix.slots + n slots, with the rows' total lengths and last rows; detach() and the
        scoring calls work on it unchanged.  A handle with `pending` ids (generate(return_prefix=True)) gets each row's pending id
        in front of its suffix, so empty suffix rows ([R, 0] ids or an all-zero mask) are legal there: that "seals" the handle."""
        if input_ids is None:
            raise ValueError("cache_prefix() needs input ids")
        if prefix is not None:
            embeds, call = self._suffix_behind(prefix, prefix_rows, input_ids, attention_mask, seq, seq_embedding, protein_tokens, 1)
            R, n, H = embeds.shape
            s = self._enter()
            with torch.cuda.stream(self._stream):
                last = torch.empty((R, H), dtype=torch.float32, device=self.device)
                logits = torch.empty((R, self.cfg.dec_vocab), dtype=torch.float32, device=self.device) if last_logits else None
                epoch = C.c_int64(0)
                _cabi.check(self._lib.opus_llama_prefix_behind(self._ctx, call.snap, embeds.data_ptr(), R, n, call.lens, call.src,
                                                               None if logits is None else logits.data_ptr(), last.data_ptr(),
                                                               C.byref(epoch), s))
            self._leave()
            lengths = torch.from_numpy(np.asarray(call.prefix_len, dtype=np.int64) + np.asarray(call.lens[:], dtype=np.int64))
            handle = OpusPrefix(self, epoch.value, last, lengths, slots=call.Tp + n)
            handle.last_logits = logits
            return handle.detach() if detach else handle
        if attention_mask is not None and not bool(attention_mask.detach().bool()[:, -1].all()):
            raise ValueError("cache_prefix(): the last slot of every row must be a real token (left-pad the prompts)")
        if seq is not None or seq_embedding is not None or protein_tokens is not None:
            _, _, mask, _, embeds, _ = self.prepare_inputs_labels_for_multimodal(
                input_ids, None, attention_mask if attention_mask is not None else torch.ones_like(input_ids, dtype=torch.bool),
                None, None, seq if seq is not None else (), seq_embedding, inference_mode=True, protein_tokens=protein_tokens)
        else:
            dummy = torch.zeros((input_ids.shape[0], self.cfg.n_prot_tokens, self.cfg.dec_dim), dtype=_cabi.operand_dtype(),
                                device=self.device)
            embeds, mask, _ = self._splice(input_ids, attention_mask, dummy, True)
        mask = mask.to(self.device).to(torch.uint8).contiguous()
        if not bool(mask[:, -1].all()):
            raise ValueError("cache_prefix(): the last slot of every row must be a real token")
        B, T, H = embeds.shape
        embeds = embeds.to(self.device, _cabi.operand_dtype()).contiguous()
        s = self._enter()
        with torch.cuda.stream(self._stream):
            last = torch.empty((B, H), dtype=torch.float32, device=self.device)
            logits = torch.empty((B, self.cfg.dec_vocab), dtype=torch.float32, device=self.device) if last_logits else None
            epoch = C.c_int64(0)
            _cabi.check(self._lib.opus_llama_prefix(self._ctx, embeds.data_ptr(), mask.data_ptr(), B, T,
                                                    None if logits is None else logits.data_ptr(), last.data_ptr(),
                                                    C.byref(epoch), s))
        self._leave()
        handle = OpusPrefix(self, epoch.value, last, mask.sum(dim=1).cpu(), slots=T)
        handle.last_logits = logits          # (last_logits=True: the fp32 last-position logits [rows, V], what a refill hands on)
        return handle.detach() if detach else handle

    def export_cache(self, epoch: int, rows: int, slots: int):
        """Copy-out of the live KV cache (opus_llama_prefix_export): rows 0 .. rows - 1, slots 0 .. slots - 1 of every layer as
        (k, v, kstart) = ([layers, rows, kv heads, slots, head_dim] x 2 in the operand dtype, int32 [rows]).  `epoch`: the cache
        epoch of the prefill that filled it (OpusPrefix._epoch, prefill_logits_behind); OpusError -6 when it is stale."""
        cfg = self.cfg
        s = self._enter()
        with torch.cuda.stream(self._stream):
            shape = (cfg.dec_layers, rows, cfg.dec_kv_heads, slots, cfg.dec_head_dim)
            k = torch.empty(shape, dtype=_cabi.operand_dtype(), device=self.device)
            v = torch.empty(shape, dtype=_cabi.operand_dtype(), device=self.device)
            kst = torch.empty((rows,), dtype=torch.int32, device=self.device)
            _cabi.check(self._lib.opus_llama_prefix_export(self._ctx, int(epoch), rows, slots, k.data_ptr(), v.data_ptr(),
                                                           kst.data_ptr(), s))
        self._leave()
        torch.cuda.current_stream(self.device).synchronize()
        return k, v, kst

    def export_cache_rows(self, keep, slots: int):
        """Ragged copy-out of the cache a decode loop left (opus_llama_prefix_export_rows): row r's window kstart[r] .. T0 +
        keep[r] - 1, right-aligned in `slots` slots, zeros in front.  (k, v, kstart) = ([layers, rows, kv heads, slots, head_dim]
        x 2 in the operand dtype, int32 [rows] = slots - window length).  OpusError -6 without a prefill, -2 for a bad keep / slots."""
        cfg = self.cfg
        keep = [int(x) for x in keep]
        rows = len(keep)
        if rows < 1 or int(slots) < 1:
            raise _cabi.OpusError(-2, f"export_cache_rows: {rows} rows x {slots} slots")
        s = self._enter()
        try:
            with torch.cuda.stream(self._stream):
                shape = (cfg.dec_layers, rows, cfg.dec_kv_heads, int(slots), cfg.dec_head_dim)
                k = torch.empty(shape, dtype=_cabi.operand_dtype(), device=self.device)
                v = torch.empty(shape, dtype=_cabi.operand_dtype(), device=self.device)
                kst = torch.empty((rows,), dtype=torch.int32, device=self.device)
                _cabi.check(self._lib.opus_llama_prefix_export_rows(self._ctx, rows, (C.c_int32 * rows)(*keep), int(slots),
                                                                    k.data_ptr(), v.data_ptr(), kst.data_ptr(), s))
        finally:
            self._leave()
        torch.cuda.current_stream(self.device).synchronize()
        return k, v, kst

    def _export_answer(self, ids: torch.Tensor, eos, kstart, T0: int) -> "OpusPrefix":
        """generate(return_prefix=True): the detached handle of prompt + answer.  Row b emitted n_b ids (counted_tokens); the
        cache holds the prompt and ids 0 .. n_b - 2 (the last id was chosen, never fed), so the export keeps n_b - 1 decode
        slots per row and the last id goes into `pending`.  kstart [B], T0: the prefill the loop ran behind."""
        from .prefix import plan_export_rows
        n_b = counted_tokens(ids, eos, getattr(self, "_stop_ids", [])).cpu()
        if ids.shape[1] < 1:
            raise ValueError("generate(return_prefix=True) needs at least one generated id")
        keep = (n_b - 1).numpy()
        lengths, Tp_out, nks = plan_export_rows(kstart, T0, keep)
        k, v, kst = self.export_cache_rows(keep, Tp_out)
        h = kst.cpu().numpy().astype(np.int32)
        if not np.array_equal(h, nks):
            raise RuntimeError(f"return_prefix: the context's row windows {h.tolist()} are not the planned ones {nks.tolist()}")
        pending = ids.cpu().gather(1, (n_b - 1).view(-1, 1)).view(-1)
        return OpusPrefix._snapshot(self, k, v, kst, h, torch.from_numpy(lengths), Tp_out, pending)

    def _usable_prefix(self, prefix: "OpusPrefix", detach: bool) -> "OpusPrefix":
        """The handle a call behind `prefix` works with: a detached one as it is (any context of the same weights), a live one
        detached on the fly when the call is going to overwrite the cache (detach)."""
        if not isinstance(prefix, OpusPrefix):
            raise TypeError("needs the OpusPrefix that cache_prefix() returned")
        if prefix.detached:
            if prefix._owner.weights is not self.weights or prefix._k.device != self.device:
                raise ValueError("a detached prefix can be used from contexts of the same weights on the same device only")
            return prefix
        if detach:
            if prefix._owner is not self:
                raise _cabi.OpusError(-6, "the prefix belongs to another context: detach() it there first")
            prefix.detach()
        return prefix

    def _suffix_behind(self, prefix, prefix_rows, inputs, attention_mask, seq, seq_embedding, protein_tokens, nret: int):
        """generate(prefix=...)'s host side: strips the rows' padding, splices them right-padded, plans the offsets (prefix.py)
        and returns (embeds [R nret, n, H], _BehindCall)."""
        from .prefix import CapacityError, plan_prefill_behind
        cfg = self.cfg
        prefix = self._usable_prefix(prefix, detach=True)
        rows, src = _suffix_rows(prefix, prefix_rows, inputs, attention_mask)
        R = len(rows)
        if R * nret > cfg.max_batch:
            raise _cabi.OpusError(-2, f"generate(prefix=...): {R * nret} decoder rows, the context holds max_batch={cfg.max_batch}")
        width = max(int(row.numel()) for row in rows)
        rp = torch.zeros((R, width), dtype=torch.long)
        rm = torch.zeros((R, width), dtype=torch.bool)
        for r, row in enumerate(rows):
            rp[r, : row.numel()] = row
            rm[r, : row.numel()] = True
        has_seq = bool((rp == DEFAULT_SEQ_TOKEN_INDEX).any())
        if has_seq and width == 1:             # (the multimodal preparation passes one-token rows through unspliced)
            raise ValueError("a suffix that is the <seq> placeholder alone is not supported: put the protein into the prefix")
        if has_seq:
            _, _, mask, _, embeds, _ = self.prepare_inputs_labels_for_multimodal(
                rp, None, rm, None, None, seq if seq is not None else (), seq_embedding, inference_mode=False,
                protein_tokens=protein_tokens)
        else:
            dummy = torch.zeros((R, cfg.n_prot_tokens, cfg.dec_dim), dtype=_cabi.operand_dtype(), device=self.device)
            embeds, mask, _ = self._splice(rp, rm, dummy, False)
        lens = mask.to(torch.int64).sum(dim=1).cpu().numpy()
        if nret > 1:                           # transformers' row layout: row r N + j is the j-th sample of row r
            embeds = embeds.repeat_interleave(nret, dim=0)
            lens, src = np.repeat(lens, nret), np.repeat(src, nret)
        cc = _cabi.CConfig.from_config(cfg)
        cap = int(self._lib.opus_llama_dec_rows_cap(C.byref(cc)))
        try:
            plan = plan_prefill_behind(prefix._kstart.cpu().numpy(), prefix.slots, src, lens, int(embeds.shape[1]), cfg.max_batch,
                                       cfg.max_prompt, cap)
        except CapacityError as e:
            need = prefix.slots + int(embeds.shape[1])
            hint = f"; a context created with max_prompt >= {need} would hold it" if need > cfg.max_prompt else ""
            raise _cabi.OpusError(-2, str(e) + hint) from None
        embeds = embeds.to(self.device, _cabi.operand_dtype()).contiguous()
        call = _BehindCall(prefix, plan.lens, plan.src)
        call.new_kstart, call.prefix_len = plan.new_kstart, plan.prefix_len
        return embeds, call

    def prefill_logits_behind(self, prefix: "OpusPrefix", embeds: torch.Tensor, lens, prefix_rows=None):
        """prefill_logits() behind a prefix (opus_llama_prefill_behind): embeds [R, n, H] right-padded suffix rows with `lens`
        real positions each, row r behind prefix row prefix_rows[r].  Returns (last-position logits fp32 [R, V], cache epoch);
        decode_logits() continues it, export_cache(epoch, ...) reads the cache back.  A live prefix is detached first."""
        prefix = self._usable_prefix(prefix, detach=True)
        R, n, _ = embeds.shape
        src = np.arange(R) if prefix_rows is None else np.asarray(prefix_rows).reshape(-1)
        call = _BehindCall(prefix, np.asarray(lens).reshape(-1), src)
        embeds = embeds.to(self.device, _cabi.operand_dtype()).contiguous()
        s = self._enter()
        with torch.cuda.stream(self._stream):
            logits = torch.empty((R, self.cfg.dec_vocab), dtype=torch.float32, device=self.device)
            epoch = C.c_int64(0)
            _cabi.check(self._lib.opus_llama_prefill_behind(self._ctx, call.snap, embeds.data_ptr(), R, n, call.lens, call.src,
                                                            logits.data_ptr(), C.byref(epoch), s))
        self._leave()
        return logits, epoch.value

    @torch.no_grad()
    def score_continuations(self, prefix: "OpusPrefix", continuations, prefix_rows=None,
                            attention_mask: Optional[torch.Tensor] = None) -> "ContinuationScores":
        """Teacher-forced log-probabilities of continuations behind a cached prefix, without prefilling the prompt again.
        `continuations`: a list of 1-D id sequences (ragged) or a right-padded LongTensor [R, n] with `attention_mask`.
        `prefix_rows` [R]: the prefix row each continuation follows (repeats and any order; default: the identity when R equals
        the prefix's row count).  Returns token_logprobs fp32 [R, n] = log p(c_j | prefix, c_<j) (0 at padding; c_0 is scored
        from the prefix's last position), logprob [R] (row sums) and n_tokens [R].  Writes neither the KV cache nor the decode
        state.  A stale handle or one of another context raises OpusError -6; n > max_prompt raises -2."""
        cfg = self.cfg
        if not isinstance(prefix, OpusPrefix):
            raise TypeError("score_continuations() needs the OpusPrefix that cache_prefix() returned")
        _refuse_pending(prefix, "score_continuations()")
        prefix = self._usable_prefix(prefix, detach=False)     # (a detached handle: read from its snapshot, never stale)
        if isinstance(continuations, torch.Tensor):
            ids = continuations.detach().cpu().long()
            if ids.dim() != 2:
                raise ValueError("continuations as a tensor must be [R, n] (right-padded)")
            m = torch.ones_like(ids, dtype=torch.bool) if attention_mask is None else attention_mask.detach().cpu().bool()
            if m.shape != ids.shape:
                raise ValueError(f"attention_mask {tuple(m.shape)} does not match the continuations {tuple(ids.shape)}")
            lens = m.sum(dim=1)
            if (m != (torch.arange(ids.shape[1])[None, :] < lens[:, None])).any():
                raise ValueError("continuations must be right-padded: the mask of a row is ones, then zeros")
            ids = ids.masked_fill(~m, 0)
        else:
            rows = [torch.as_tensor(c, dtype=torch.long).reshape(-1).cpu() for c in continuations]
            lens = torch.tensor([r.numel() for r in rows], dtype=torch.long)
            ids = torch.zeros((len(rows), max([1] + lens.tolist())), dtype=torch.long)
            for i, r in enumerate(rows):
                ids[i, : r.numel()] = r
            m = torch.arange(ids.shape[1])[None, :] < lens[:, None]
        R, n = ids.shape
        if R < 1:
            raise ValueError("score_continuations() needs at least one continuation")
        if n > cfg.max_prompt:
            raise _cabi.OpusError(-2, f"score_continuations: continuations of {n} positions exceed max_prompt={cfg.max_prompt}")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= cfg.dec_vocab):
            raise ValueError(f"continuation ids must lie in [0, {cfg.dec_vocab})")
        if prefix_rows is None:
            if R != prefix.rows:
                raise ValueError(f"{R} continuations for {prefix.rows} prefix rows: pass prefix_rows")
            src = np.arange(R, dtype=np.int32)
        else:
            src = np.asarray(torch.as_tensor(prefix_rows).cpu(), dtype=np.int64).reshape(-1)
            if src.shape[0] != R:
                raise ValueError(f"prefix_rows has {src.shape[0]} entries for {R} continuations")
            if src.size and (src.min() < 0 or src.max() >= prefix.rows):
                raise ValueError(f"prefix_rows must lie in [0, {prefix.rows})")
            src = src.astype(np.int32)
        dev = self.device
        lens_np = lens.numpy().astype(np.int32)
        tgt = ids[m].to(torch.int32)                                       # compact: row-major over the real tokens
        N = int(tgt.numel())
        cc = _cabi.CConfig.from_config(cfg)
        n_scratch = int(self._lib.opus_llama_score_scratch_bytes(C.byref(cc), R, n))
        if n_scratch < 0:
            raise _cabi.OpusError(-2, f"score_continuations: R={R} n={n}")
        embeds = self.model.embed_tokens(ids.to(dev)).to(_cabi.operand_dtype()).contiguous()
        s = self._enter()
        with torch.cuda.stream(self._stream):
            scratch = torch.empty((n_scratch,), dtype=torch.uint8, device=dev)
            d_tgt = tgt.to(dev, non_blocking=True) if N else torch.zeros((1,), dtype=torch.int32, device=dev)
            lp = torch.zeros((max(N, 1),), dtype=torch.float32, device=dev)
            h_lens = (C.c_int32 * R)(*lens_np.tolist())
            h_src = (C.c_int32 * R)(*src.tolist())
            if prefix.detached:                # the same pass reading the snapshot: no epoch, the cache is not touched
                snap = prefix._snap()
                _cabi.check(self._lib.opus_llama_score_continuations_detached(
                    self._ctx, C.byref(snap), embeds.data_ptr(), R, n, h_lens, h_src, prefix._last_rows.data_ptr(),
                    d_tgt.data_ptr(), lp.data_ptr(), scratch.data_ptr(), n_scratch, s))
            else:
                _cabi.check(self._lib.opus_llama_score_continuations(
                    self._ctx, embeds.data_ptr(), R, n, h_lens, h_src, prefix._last_rows.data_ptr(), prefix.rows, prefix._epoch,
                    d_tgt.data_ptr(), lp.data_ptr(), scratch.data_ptr(), n_scratch, s))
            token_lp = torch.zeros((R, n), dtype=torch.float32, device=dev)
            token_lp[m.to(dev)] = lp[:N]
            logprob = token_lp.sum(dim=1)
        self._leave()
        return ContinuationScores(token_lp, logprob, lens.to(dev))

    # ------------------------------------------------------------------ trie scoring
    @torch.no_grad()
    def score_trie(self, prefix: "OpusPrefix", trie, include_stop: bool = False) -> "TrieScores":
        """Exact log-probabilities of EVERY member of a TokenTrie behind a cached prefix, in one tree pass: each trie node is one
        new decoder position that attends to the cached prompt and to its own ancestors, and a member's log-prob is the sum of
        the edge log-probs on its path - what score_continuations(prefix, [member_ids[m]], prefix_rows=[p]).logprob gives, without
        re-computing the shared token prefixes once per member.  `trie`: a TokenTrie (every prefix row scores it) or
        TokenTrie.per_row([...]) with one trie per prefix row.  include_stop adds log sum_{s in S} p(s | prompt + member), S = the
        trie's end ids (+ the separator's first id): what the constraint allows in a completing state besides the children; it
        costs one decoder row per leaf (without it only the nodes that have a child are evaluated).  Returns TrieScores.  Reads
        the KV cache, writes neither it nor the decode state.  A stale handle or one of another context raises OpusError -6; a
        member deeper than constraint.TRIE_MAX_DEPTH or a path beyond max_prompt + max_new_tokens positions raises -2."""
        from .constraint import PerRowTokenTrie, TokenTrie, TRIE_MAX_DEPTH, plan_trie_score
        cfg = self.cfg
        if not isinstance(prefix, OpusPrefix):
            raise TypeError("score_trie() needs the OpusPrefix that cache_prefix() returned")
        _refuse_pending(prefix, "score_trie()")
        prefix = self._usable_prefix(prefix, detach=False)     # (a detached handle: read from its snapshot, never stale)
        if isinstance(trie, TokenTrie):
            tries = [trie] * prefix.rows
        elif isinstance(trie, PerRowTokenTrie):
            if trie.n_rows() != prefix.rows:
                raise ValueError(f"TokenTrie.per_row of {trie.n_rows()} tries for {prefix.rows} prefix rows")
            tries = list(trie.tries)
        else:
            raise TypeError("score_trie() needs a TokenTrie or TokenTrie.per_row(...)")
        deepest = max(t.max_depth for t in tries)
        if deepest > TRIE_MAX_DEPTH:
            raise _cabi.OpusError(-2, f"score_trie: a member of {deepest} ids, the depth limit is {TRIE_MAX_DEPTH}")
        ctx_cap = cfg.max_prompt + cfg.max_new_tokens
        for p, t in enumerate(tries):
            if int(prefix.lengths[p]) + t.max_depth > ctx_cap:
                raise _cabi.OpusError(-2, f"score_trie: prompt of {int(prefix.lengths[p])} tokens + a member of {t.max_depth} ids exceed "
                                          f"the context's {ctx_cap} positions (max_prompt + max_new_tokens)")
            if max(max(t.node_tok), max(t.stop_ids())) >= cfg.dec_vocab:
                raise ValueError(f"trie ids must lie in [0, {cfg.dec_vocab})")
        cc = _cabi.CConfig.from_config(cfg)
        cap = int(self._lib.opus_llama_dec_rows_cap(C.byref(cc)))
        if cap < 1:
            raise _cabi.OpusError(-2, "score_trie: bad config")
        key = (prefix.rows, bool(include_stop), cap)                     # (a trie does not change after construction)
        if key not in trie._score_plans:
            trie._score_plans[key] = plan_trie_score(tries, include_stop, cap)
        plan = trie._score_plans[key]
        P, N, M, dev = plan.P, plan.N, plan.M, self.device
        ptr = lambda a: a.ctypes.data if a.size else None                # noqa: E731
        s = self._enter()
        with torch.cuda.stream(self._stream):
            node_lp = torch.zeros((P, N + 1), dtype=torch.float32, device=dev)
            stop_node = torch.full((P, N + 1), float("-inf"), dtype=torch.float32, device=dev) if include_stop else None
            for ps in plan.passes:
                n_sets = len(plan.tries) if ps.stop_row.size else 0
                n_ids = int(plan.stop_ids.size) if ps.stop_row.size else 0
                n_scratch = int(self._lib.opus_llama_score_tree_scratch_bytes(C.byref(cc), ps.rows, ps.score_src.size, ps.edge_row.size,
                                                                              ps.stop_row.size, n_ids, n_sets))
                if n_scratch < 0:
                    raise _cabi.OpusError(-2, f"score_trie: a pass of {ps.rows} rows")
                scratch = torch.empty((n_scratch,), dtype=torch.uint8, device=dev)
                emb = None
                if ps.rows:
                    emb = self.model.embed_tokens(torch.from_numpy(ps.tok.astype(np.int64)).to(dev)).to(_cabi.operand_dtype()).contiguous()
                head = (emb.data_ptr() if emb is not None else None, ps.rows, ptr(ps.prow), ptr(ps.parent), ptr(ps.depth),
                        ps.score_src.size, ptr(ps.score_src), ps.edge_row.size, ptr(ps.edge_row), ptr(ps.edge_tok), ptr(ps.edge_slot),
                        ps.stop_row.size, ptr(ps.stop_row), ptr(ps.stop_set), ptr(ps.stop_slot), n_ids, ptr(plan.stop_ids), n_sets,
                        ptr(plan.stop_off), prefix._last_rows.data_ptr())
                tail = (node_lp.data_ptr(), stop_node.data_ptr() if include_stop else None, P * (N + 1), scratch.data_ptr(),
                        n_scratch, s)
                if prefix.detached:            # the same pass reading the snapshot: no epoch, the cache is not touched
                    snap = prefix._snap()
                    _cabi.check(self._lib.opus_llama_score_tree_detached(self._ctx, C.byref(snap), *head, *tail))
                else:
                    _cabi.check(self._lib.opus_llama_score_tree(self._ctx, *head, P, prefix._epoch, *tail))
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
            trie_of_row, member_node = d(plan.trie_of_row), d(plan.member_node)
            par, depth = d(plan.node_par), d(plan.node_depth)
            member_lp = torch.empty((P, M), dtype=torch.float32, device=dev)
            _cabi.check(self._lib.opus_trie_path_sums(self._ctx, node_lp.data_ptr(), trie_of_row.data_ptr(), par.data_ptr(),
                                                      depth.data_ptr(), member_node.data_ptr(), P, M, N + 1, member_lp.data_ptr(), s))
            stop_lp = None
            if include_stop:
                mn = member_node[trie_of_row.long()].long()                      # [P, M], -1 beyond a row's members
                stop_lp = torch.gather(stop_node, 1, mn.clamp(min=0)).masked_fill(mn < 0, float("-inf"))
            torch.cuda.current_stream().synchronize()
        self._leave()
        return TrieScores(member_lp, stop_lp, node_lp, torch.from_numpy(plan.n_members).to(dev), plan.rows_evaluated)

    # ------------------------------------------------------------------ trie search
    def _set_trie_search(self, trie):
        """The search table of `trie` (constraint.TrieSearchTable, kept on the trie object), uploaded to this context unless it
        is the one the context holds."""
        from .constraint import TrieSearchTable
        tab = getattr(trie, "_search_table", None)
        if tab is None:
            tab = trie._search_table = TrieSearchTable(trie.tries if hasattr(trie, "tries") else [trie])
        if getattr(self, "_trie_search", None) is not tab:
            p = lambda a: a.ctypes.data                                                      # noqa: E731
            s = self._enter()
            try:
                _cabi.check(self._lib.opus_set_trie_search(self._ctx, tab.n_states, p(tab.edge_off), p(tab.edge_tok), p(tab.edge_next),
                                                           tab.n_edges, p(tab.member), p(tab.stop_set), len(tab.stop_off) - 1,
                                                           p(tab.stop_off), p(tab.stop_ids), s))
            finally:
                self._leave()
            self._trie_search = tab
        return tab

    @torch.no_grad()
    def search_trie(self, prefix: "OpusPrefix", trie, num_beams: int = 8, top: int = 5, include_stop: bool = False,
                    return_trace: bool = False) -> "TrieSearchResult":
        """The `top` best members of a TokenTrie behind a cached prefix, by beam search over the trie with `num_beams` beams per
        prompt: score_trie()'s scores and member numbering at num_beams x depth decoder rows per prompt instead of one row per
        trie node.  `trie`: a TokenTrie (every prefix row searches it) or TokenTrie.per_row([...]).  Returns TrieSearchResult.

        Scores are score_trie()'s: a member's log-prob is the sum of its edge log-probs behind prompt p, added in fp32 from the
        root; include_stop adds the log of the mass on TokenTrie.stop_ids() at the member's node.

        The search is level-synchronous, per prompt.  The frontier starts as {root, 0}; the prefix's last-position logits serve
        level 1 without a decoder pass.  At each level every live beam (node s, score a) offers its children with a + logp(id).
        Without include_stop a child that is a member goes to the pool of finished members at once and only children that have a
        child compete for the num_beams slots (a leaf is never run through the decoder); with it every child competes and a beam
        standing on a member node adds score + stop term to the pool at the next level, from its own logits.  Beams are chosen
        by score descending, ties to the lower (beam, id); the pool keeps the best `top`, ties to the lower member index.  A
        prompt stops when it has no live beam or when its best beam is STRICTLY below its top-th pool entry (every term is
        <= 0: exact).  `exhaustive[p]` says that no candidate of prompt p ever went without a slot: the row then equals
        score_trie(...).topk(top) up to the two launch shapes' rounding; otherwise it is approximate - a member whose prefix fell
        out of the beam is missed.

        Each level is one launch (trie_beam_expand_kernel) that leaves ids, parent rows, states, scores and the pool on the
        device; the host reads two words per level.  P x num_beams decoder rows above max_batch run as groups of
        max_batch // num_beams prompts.  The call overwrites the context's decode rows and KV cache as generate(prefix=...) does:
        a live handle is detached first, other live handles go stale.

        ValueError: 1 <= top <= num_beams <= 16 violated; a trie deeper than the context's max_new_tokens or
        constraint.TRIE_MAX_DEPTH; num_beams > max_batch; a prefix as wide as max_prompt (the beams' first pass needs one slot)."""
        from .constraint import PerRowTokenTrie, TokenTrie, TRIE_MAX_DEPTH, TRIE_SEARCH_MAX_BEAMS
        cfg = self.cfg
        if not isinstance(prefix, OpusPrefix):
            raise TypeError("search_trie() needs the OpusPrefix that cache_prefix() returned")
        _refuse_pending(prefix, "search_trie()")
        if isinstance(trie, TokenTrie):
            tries = [trie] * prefix.rows
        elif isinstance(trie, PerRowTokenTrie):
            if trie.n_rows() != prefix.rows:
                raise ValueError(f"TokenTrie.per_row of {trie.n_rows()} tries for {prefix.rows} prefix rows")
            tries = list(trie.tries)
        else:
            raise TypeError("search_trie() needs a TokenTrie or TokenTrie.per_row(...)")
        K, top = int(num_beams), int(top)
        if not 1 <= top <= K <= TRIE_SEARCH_MAX_BEAMS:
            raise ValueError(f"search_trie: 1 <= top <= num_beams <= {TRIE_SEARCH_MAX_BEAMS} (got top={top}, num_beams={K})")
        deepest = max(t.max_depth for t in tries)
        if deepest > TRIE_MAX_DEPTH:
            raise ValueError(f"search_trie: a member of {deepest} ids, the depth limit is TRIE_MAX_DEPTH={TRIE_MAX_DEPTH}")
        if deepest > cfg.max_new_tokens:
            raise ValueError(f"search_trie: a member of {deepest} ids, the context decodes max_new_tokens={cfg.max_new_tokens}")
        if K > cfg.max_batch:
            raise ValueError(f"search_trie: num_beams={K} decoder rows per prompt need max_batch>={K} (the context holds {cfg.max_batch})")
        if prefix.slots + 1 > cfg.max_prompt:
            raise ValueError(f"search_trie: a prefix of {prefix.slots} slots + the beams' first id exceed max_prompt={cfg.max_prompt}")
        for t in tries:
            if max(max(t.node_tok), max(t.stop_ids())) >= cfg.dec_vocab:
                raise ValueError(f"trie ids must lie in [0, {cfg.dec_vocab})")
        prefix = self._usable_prefix(prefix, detach=True)
        tab = self._set_trie_search(trie)
        P, dev, H = prefix.rows, self.device, cfg.dec_dim
        per = cfg.max_batch // K                                            # prompts per group
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        pool_m = torch.full((P, top), -1, **i32)
        pool_lp = torch.full((P, top), float("-inf"), **f32)
        pool_st = torch.full((P, top), float("-inf"), **f32)
        flags = torch.tensor([1, 1, 0], **i32).repeat(P, 1).contiguous()
        start = torch.from_numpy(tab.start).to(dev).expand(P).contiguous()  # (one trie for every row: one start state)
        snap = prefix._snap()
        levels, rows_decoded, trace = 0, 0, []
        s = self._enter()
        with torch.cuda.stream(self._stream):
            for p0 in range(0, P, per):
                g = min(per, P - p0)
                R = g * K
                state = torch.zeros((g, K), **i32)
                state[:, 0] = start[p0: p0 + g]
                score = torch.full((g, K), float("-inf"), **f32)
                score[:, 0] = 0.0
                tok, parent, words = torch.zeros((R,), **i32), torch.zeros((R,), **i32), torch.zeros((2,), **i32)
                lse = torch.empty((R,), **f32)
                edge_lp = torch.empty((g, K), **f32) if return_trace else None
                beam_stop = torch.empty((g, K), **f32) if return_trace else None
                ptr = lambda x: None if x is None else x.data_ptr()                          # noqa: E731
                io = _cabi.CTrieSearchIO(g, K, top, 1 if include_stop else 0, state.data_ptr(), score.data_ptr(), tok.data_ptr(),
                                         parent.data_ptr(), pool_m[p0:].data_ptr(), pool_lp[p0:].data_ptr(), pool_st[p0:].data_ptr(),
                                         flags[p0:].data_ptr(), words.data_ptr(), lse.data_ptr(), ptr(edge_lp), ptr(beam_stop))
                h_lens = (C.c_int32 * R)(*([1] * R))
                h_src = (C.c_int32 * R)(*[p0 + r // K for r in range(R)])
                _cabi.check(self._lib.opus_trie_search_begin(self._ctx, prefix._last_rows[p0: p0 + g].contiguous().data_ptr(), g, s))
                n = 0
                while True:
                    before = state.clone() if return_trace else None
                    _cabi.check(self._lib.opus_trie_search_level(self._ctx, C.byref(io), 1 if n == 0 else 0, s))
                    n += 1
                    live, moved = words.cpu().tolist()                                       # (synchronises this stream)
                    if return_trace:
                        trace.append(dict(group=p0, level=n, prompt=p0 + torch.arange(g).repeat_interleave(K),
                                          node=(state - start[p0: p0 + g, None]).clamp(min=0).cpu().reshape(-1), alive=(state > 0).cpu().reshape(-1),
                                          edge_logprob=edge_lp.cpu().reshape(-1), score=score.cpu().reshape(-1),
                                          from_node=(before - start[p0: p0 + g, None]).clamp(min=0).cpu().reshape(-1),
                                          from_alive=(before > 0).cpu().reshape(-1), from_stop=beam_stop.cpu().reshape(-1)))
                    if not live:
                        break
                    if n > deepest:                                                          # (level depth + 1 offers stop terms only)
                        raise _cabi.OpusError(-1, "search_trie: the search ran past the trie's depth")
                    if n == 1:
                        emb = self.model.embed_tokens(tok.long()).to(_cabi.operand_dtype()).view(R, 1, H).contiguous()
                        _cabi.check(self._lib.opus_llama_prefill_behind(self._ctx, C.byref(snap), emb.data_ptr(), R, 1, h_lens, h_src,
                                                                        None, None, s))
                    else:
                        if moved:
                            _cabi.check(self._lib.opus_kv_reorder(self._ctx, parent.data_ptr(), R, s))
                        _cabi.check(self._lib.opus_llama_decode_step(self._ctx, tok.data_ptr(), None, s))
                    rows_decoded += R
                levels = max(levels, n)
            torch.cuda.current_stream().synchronize()
        self._leave()
        n_members = torch.as_tensor([len(t.member_ids) for t in tries], device=dev)
        return TrieSearchResult(pool_m.long(), pool_lp, pool_st if include_stop else None, levels, rows_decoded, flags[:, 1].bool(),
                                n_members, trace if return_trace else None)

    # ------------------------------------------------------------------ parity taps (tests / bench)
    def prefill_logits(self, embeds: torch.Tensor, mask: torch.Tensor, num_return_sequences: int = 1) -> torch.Tensor:
        """Last-position logits fp32 [B, V].  num_return_sequences = N > 1: the fanned-out prefill (opus_llama_prefill_fanout) -
        [B N, V], row b N + j = prompt b, and decode_logits() then takes B N tokens."""
        B, T, _ = embeds.shape
        N = int(num_return_sequences)
        embeds = embeds.to(self.device, _cabi.operand_dtype()).contiguous()
        mask = mask.to(self.device).to(torch.uint8).contiguous()
        s = self._enter()
        with torch.cuda.stream(self._stream):
            logits = torch.empty((B * max(N, 1), self.cfg.dec_vocab), dtype=torch.float32, device=self.device)
            if N != 1:
                _cabi.check(self._lib.opus_llama_prefill_fanout(self._ctx, embeds.data_ptr(), mask.data_ptr(), B, T, N,
                                                                logits.data_ptr(), s))
            else:
                _cabi.check(self._lib.opus_llama_prefill(self._ctx, embeds.data_ptr(), mask.data_ptr(), B, T,
                                                         logits.data_ptr(), s))
        self._leave()
        return logits

    def decode_logits(self, tok: torch.Tensor) -> torch.Tensor:
        tok = tok.to(self.device, torch.int32).contiguous()
        s = self._enter()
        with torch.cuda.stream(self._stream):
            logits = torch.empty((tok.shape[0], self.cfg.dec_vocab), dtype=torch.float32, device=self.device)
            _cabi.check(self._lib.opus_llama_decode_step(self._ctx, tok.data_ptr(), logits.data_ptr(), s))
        self._leave()
        return logits

    def last_hidden(self, B: int, T: int) -> torch.Tensor:
        s = self._enter()
        with torch.cuda.stream(self._stream):
            h = torch.empty((B, T, self.cfg.enc_dim), dtype=torch.float32, device=self.device)
            _cabi.check(self._lib.opus_esm2_last_hidden(self._ctx, h.data_ptr(), B, T, s))
        self._leave()
        return h

    # ------------------------------------------------------------------ measurement
    def timing(self, on: bool):
        _cabi.check(self._lib.opus_timing_enable(self._ctx, 1 if on else 0))
        _cabi.check(self._lib.opus_timing_reset(self._ctx))

    def timing_get(self, klass: str = "*", phase: str = "*"):
        """(ms, launches, algorithmic bytes, algorithmic flops) of the recorded launches matching class and phase."""
        ms, n, by, fl = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        _cabi.check(self._lib.opus_timing_get(self._ctx, klass.encode(), phase.encode(), C.byref(ms), C.byref(n), C.byref(by),
                                              C.byref(fl)))
        return ms.value, n.value, by.value, fl.value

    def timing_names(self):
        buf = C.create_string_buffer(512)
        _cabi.check(self._lib.opus_timing_names(buf, 512))
        classes, phases = buf.value.decode().split(";")
        return classes.split(","), phases.split(",")

    def drop_decode_graphs(self) -> None:
        """Forget the captured decode steps of this context (measurement aid: what a capture + instantiation per batch costs)."""
        _cabi.check(self._lib.opus_debug_knob(self._ctx, b"misc0", 0))

    def stat(self, name: str) -> int:
        """Counters of this context: "graph_instantiations" (decode-step hipGraphs instantiated: one per distinct batch size /
        token budget / sampling setting, none per prompt length), "graph_replays", "graphs_cached"."""
        v = int(self._lib.opus_stat(self._ctx, name.encode()))
        if v < 0:
            raise KeyError(name)
        return v

    def last_logits(self, B: int) -> torch.Tensor:
        """fp32 [B, V] logits of the most recent prefill / decode step (the optional logits gather of SURVEY 8e)."""
        s = self._enter()
        with torch.cuda.stream(self._stream):
            out = torch.empty((B, self.cfg.dec_vocab), dtype=torch.float32, device=self.device)
            _cabi.check(self._lib.opus_last_logits(self._ctx, out.data_ptr(), B, s))
        self._leave()
        return out


def _splice_labels(input_ids, attention_mask, labels, n_tok, T_out, inference_mode):
    """Label bookkeeping of opus_arch.py:172-233,255,266 (training-side only; host integer logic)."""
    ids = input_ids.cpu()
    lab = labels.cpu()
    m = torch.ones_like(ids, dtype=torch.bool) if attention_mask is None else attention_mask.cpu().bool()
    out = torch.full((ids.shape[0], T_out), IGNORE_INDEX, dtype=lab.dtype)
    for b in range(ids.shape[0]):
        row: List[int] = []
        for t in range(ids.shape[1]):
            if not m[b, t]:
                continue
            if int(ids[b, t]) == DEFAULT_SEQ_TOKEN_INDEX:
                row.extend([IGNORE_INDEX] * n_tok)
            else:
                row.append(int(lab[b, t]))
        row = row[:T_out]
        if row:
            if inference_mode:
                out[b, T_out - len(row):] = torch.tensor(row, dtype=lab.dtype)
            else:
                out[b, : len(row)] = torch.tensor(row, dtype=lab.dtype)
    return out


def _check_forward_mask(m: np.ndarray, pos: Optional[np.ndarray]) -> None:
    """The rows forward() can score as HF would: the valid slots of every row are contiguous; a row that starts late (left
    padding) needs position_ids == cumsum(mask) - 1 on its real slots, which is what the kernels compute (t - first valid slot)
    and not what HF derives without position_ids (arange).  Given position_ids must equal that on every real slot."""
    B, T = m.shape
    for b in range(B):
        idx = np.flatnonzero(m[b])
        if idx.size and idx[-1] - idx[0] + 1 != idx.size:
            raise ValueError(f"attention_mask row {b} has a hole: valid slots must be contiguous (right- or left-padded rows)")
    want = np.cumsum(m, axis=1) - 1
    if pos is not None:
        if pos.shape != (B, T):
            raise ValueError(f"position_ids {pos.shape} do not match the mask {(B, T)}")
        if (pos != want)[m].any():
            raise ValueError("position_ids must equal cumsum(attention_mask) - 1 on the real slots: the kernels derive positions "
                             "from the mask")
    elif (m.any(axis=1) & ~m[:, 0]).any():
        raise ValueError("left-padded rows need position_ids = cumsum(attention_mask) - 1: without them HF uses arange positions "
                         "and the result would differ; pass position_ids or right-pad the rows")


class OpusPrefix:
    """What cache_prefix() returns: a prompt batch prefilled into its context's KV cache.  `rows` prompts, `lengths` [rows] their
    real token counts; the final residual row of every prompt's last position (fp32 [rows, hidden]) scores a continuation's first
    token.  Valid until the next call on the context that prefills or permutes its cache (the epoch check of the native side)."""

    def __init__(self, owner, epoch: int, last_rows: torch.Tensor, lengths: torch.Tensor, slots: int = 0):
        self._owner, self._epoch, self._last_rows = owner, int(epoch), last_rows
        self.rows = int(last_rows.shape[0]) if last_rows is not None else int(lengths.shape[0])
        self.lengths = lengths
        self.slots = int(slots)          # Tp: cache slots per row (the padded prompt width)
        self._k = self._v = self._kstart = self._h_kstart = None
        # generate(return_prefix=True): int64 [rows], the last id every row emitted - chosen, never fed, so its K / V is not in
        # the snapshot and the handle has no last rows.  generate(prefix=) and cache_prefix(prefix=) feed it in front of the
        # suffix; the scoring calls need a sealed handle (cache_prefix(prefix=handle)).  None on every other handle.
        self.pending = None

    @classmethod
    def _snapshot(cls, owner, k, v, kstart, h_kstart, lengths, slots: int, pending) -> "OpusPrefix":
        """A detached handle around an export of the live cache (generate(return_prefix=True))."""
        self = cls(owner, -1, None, lengths, slots)
        self._k, self._v, self._kstart = k, v, kstart
        self._h_kstart = (C.c_int32 * self.rows)(*[int(x) for x in h_kstart])
        self.pending = pending
        return self

    def nbytes(self) -> int:
        """Device bytes a detached handle holds in K and V (prefix.snapshot_bytes); 0 for a live one."""
        return 0 if self._k is None else int(self._k.numel() * self._k.element_size() * 2)

    @property
    def detached(self) -> bool:
        return self._k is not None

    def detach(self) -> "OpusPrefix":
        """Copies the rows' K and V of all layers out of the context's cache into tensors this handle owns
        ([layers][rows][kv heads][slots][head_dim], operand dtype; beside them kstart [rows] and the fp32 last rows it already
        keeps) and returns the handle.  A detached handle never goes stale, can be used any number of times by generate(prefix=),
        score_continuations() and score_trie(), and by new_context() contexts of the same weights.  OpusError -6 when the live
        handle is already stale; a second detach() is a no-op."""
        if not self.detached:
            k, v, kst = self._owner.export_cache(self._epoch, self.rows, self.slots)
            h = kst.cpu().numpy().astype(np.int32)
            self._k, self._v, self._kstart = k, v, kst
            self._h_kstart = (C.c_int32 * self.rows)(*h.tolist())
        return self

    def _snap(self) -> "_cabi.CPrefixSnap":
        return _cabi.CPrefixSnap(self._k.data_ptr(), self._v.data_ptr(), self._kstart.data_ptr(), self._h_kstart, self.rows, self.slots)


def _refuse_pending(prefix: OpusPrefix, who: str) -> None:
    if prefix.pending is not None:
        raise ValueError(f"{who}: the handle holds pending ids (the last id of every answer was chosen but never fed, so it has no "
                         f"last rows to score from): seal it with cache_prefix(prefix=handle)")


def _suffix_rows(prefix, prefix_rows, inputs, attention_mask):
    """The unpadded suffix rows of a call behind `prefix` (1-D int64 tensors) and the prefix row of each (int64 [R]).  A handle
    with `pending` ids (generate(return_prefix=True)) gets the pending id of row prefix_rows[r] in front of suffix row r, so an
    empty suffix row is legal there; behind any other handle it is a ValueError."""
    ids = inputs.detach().cpu().long()
    if ids.dim() != 2:
        raise ValueError("generate(prefix=...) takes suffix ids [R, n]")
    m = torch.ones_like(ids, dtype=torch.bool) if attention_mask is None else attention_mask.detach().cpu().bool()
    rows = [ids[r][m[r]] for r in range(ids.shape[0])]
    R = len(rows)
    pending = getattr(prefix, "pending", None)
    if pending is None:
        for r, row in enumerate(rows):
            if row.numel() == 0:
                raise ValueError(f"suffix row {r} is empty: every row needs at least one token behind the prefix")
    if prefix_rows is None:
        if R != prefix.rows:
            raise ValueError(f"{R} suffix rows for {prefix.rows} prefix rows: pass prefix_rows")
        src = np.arange(R, dtype=np.int64)
    else:
        src = np.asarray(torch.as_tensor(prefix_rows).cpu(), dtype=np.int64).reshape(-1)
        if src.shape[0] != R:
            raise ValueError(f"prefix_rows has {src.shape[0]} entries for {R} suffix rows")
    if pending is not None:
        if src.size and (src.min() < 0 or src.max() >= prefix.rows):
            raise ValueError(f"prefix_rows must lie in [0, {prefix.rows})")
        pend = pending.detach().cpu().long()
        rows = [torch.cat([pend[int(p)].view(1), row]) for row, p in zip(rows, src)]
    return rows, src


class _BehindCall:
    """Arguments of one opus_*_behind call (kept alive for its duration): the snapshot, the rows' lengths and prefix rows."""

    def __init__(self, prefix: OpusPrefix, lens: np.ndarray, src: np.ndarray):
        self.prefix, self.Tp = prefix, prefix.slots
        self.new_kstart = None           # (set by _suffix_behind: the decode rows' first real slots, prefix.plan_prefill_behind)
        self._struct = prefix._snap()
        self.snap = C.byref(self._struct)
        self.lens = (C.c_int32 * len(lens))(*[int(x) for x in lens])
        self.src = (C.c_int32 * len(src))(*[int(x) for x in src])


def _take(x, group):
    """Entries `group` of a per-prompt argument (None, a list or a tensor)."""
    if x is None:
        return None
    if torch.is_tensor(x):
        return x[torch.as_tensor(list(group), dtype=torch.long, device=x.device)]
    picked = [x[p] for p in group]
    return torch.stack(picked) if picked and torch.is_tensor(picked[0]) else picked


class _StreamBackend:
    """The device side of continuous.run_schedule(): sessions on the model's context (opus_stream_*), refill groups prefilled
    in the model's helper context (cache_prefix(detach=True, last_logits=True))."""

    def __init__(self, model, prompts, lens, seqs, seq_embedding, protein_tokens, max_new, eos, pad_id, sampler, slots):
        self.m, self.prompts, self.lens = model, prompts, lens
        self.seqs, self.seq_embedding, self.protein_tokens = seqs, seq_embedding, protein_tokens
        self.max_new, self.eos, self.pad_id, self.sampler = max_new, eos, pad_id, sampler
        self.dev: List[Optional[torch.Tensor]] = [None] * len(prompts)
        cfg = model.cfg
        with torch.cuda.stream(model._stream):
            # one persistent id buffer [max_batch, S]: its address is part of the captured step's identity
            if getattr(model, "_stream_ids", None) is None:
                model._stream_ids = torch.empty((cfg.max_batch, cfg.max_new_tokens), dtype=torch.int32, device=model.device)
        self.ids = model._stream_ids
        self.B = 0

    def _kw(self, group):
        kw = dict(seq_embedding=_take(self.seq_embedding, group), protein_tokens=_take(self.protein_tokens, group))
        seq = _take(self.seqs, group)
        return seq, kw

    def begin(self, prompts, T0):
        m = self.m
        ids, mask = _left_pack([self.prompts[p].tolist() for p in prompts])
        seq, kw = self._kw(prompts)
        if seq is not None or kw["seq_embedding"] is not None or kw["protein_tokens"] is not None:
            _, _, mask, _, embeds, _ = m.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, seq if seq is not None else (),
                                                                              kw["seq_embedding"], inference_mode=True,
                                                                              protein_tokens=kw["protein_tokens"])
        else:
            dummy = torch.zeros((len(prompts), m.cfg.n_prot_tokens, m.cfg.dec_dim), dtype=_cabi.operand_dtype(), device=m.device)
            embeds, mask, _ = m._splice(ids, mask, dummy, True)
        if int(embeds.shape[1]) != T0:
            raise RuntimeError(f"the splice gave {int(embeds.shape[1])} positions, the schedule planned {T0}")
        embeds = embeds.contiguous()
        mask = mask.to(m.device).to(torch.uint8).contiguous()
        self.B = len(prompts)
        t, p, sd = (self.sampler[0], self.sampler[1], self.sampler[2]) if self.sampler is not None else (0.0, 1.0, 0)
        eos_arr = (C.c_int32 * max(1, len(self.eos)))(*self.eos)
        s = m._enter()
        with torch.cuda.stream(m._stream):
            self.ids.fill_(self.pad_id)
            _cabi.check(m._lib.opus_stream_begin(m._ctx, embeds.data_ptr(), mask.data_ptr(), self.B, T0, self.max_new, eos_arr,
                                                 len(self.eos), self.pad_id, t, p, sd, self.ids.data_ptr(), s))
        m._leave()

    def run(self, t_min, min_free, t_max):
        m = self.m
        t_out, h_end = C.c_int32(0), (C.c_int32 * self.B)()
        _cabi.check(m._lib.opus_stream_run(m._ctx, int(t_min), int(min_free), int(t_max), C.byref(t_out), h_end, m._stream.cuda_stream))
        return t_out.value, list(h_end)

    def harvest(self, prompt, row, start, end):
        with torch.cuda.stream(self.m._stream):          # (stream-ordered in front of the refill that clears the row's tail)
            self.dev[prompt] = self.ids[row, start:end + 1].clone()

    def refill(self, assign, t, L):
        m = self.m
        if getattr(m, "_helper", None) is None:
            m._helper = m.new_context()
        group = [p for _, p in assign]
        ids, mask = _left_pack([self.prompts[p].tolist() for p in group])
        seq, kw = self._kw(group)
        h = m._helper.cache_prefix(ids, seq=seq, attention_mask=mask, detach=True, last_logits=True, **kw)
        n = len(group)
        rows = (C.c_int32 * n)(*[r for r, _ in assign])
        src = (C.c_int32 * n)(*range(n))
        lens = (C.c_int32 * n)(*[self.lens[p] for p in group])
        snap = h._snap()
        s = m._enter()
        for x in (h._k, h._v, h._kstart, h.last_logits):  # allocated on the helper's stream, read on this context's
            x.record_stream(m._stream)
        _cabi.check(m._lib.opus_stream_refill(m._ctx, C.byref(snap), n, rows, src, h.last_logits.data_ptr(), lens, s))
        m._leave()

    def finish(self):
        m = self.m
        h_end = (C.c_int32 * self.B)()
        s = m._enter()
        _cabi.check(m._lib.opus_stream_end(m._ctx, h_end, s))
        m._leave()
        return list(h_end)

    def results(self):
        self.m._stream.synchronize()
        return [x.long().cpu() for x in self.dev]


class ContinuousOutput:
    """generate_continuous(return_dict_in_generate=True): `sequences` (N 1-D int64 tensors, input order), `n_tokens` int64 [N],
    `stats` (sessions, decode_steps, refills, rows_refilled, live_row_steps, slot_steps)."""

    def __init__(self, sequences, n_tokens, stats):
        self.sequences, self.n_tokens, self.stats = sequences, n_tokens, stats


class ContinuationScores:
    """What score_continuations() returns: token_logprobs fp32 [R, n] (0 at padding), logprob fp32 [R] (row sums), n_tokens [R]."""

    def __init__(self, token_logprobs: torch.Tensor, logprob: torch.Tensor, n_tokens: torch.Tensor):
        self.token_logprobs, self.logprob, self.n_tokens = token_logprobs, logprob, n_tokens


class TrieScores:
    """What score_trie() returns.  member_logprob fp32 [P, M] = log p(member's tokens | prompt p); stop_logprob [P, M] (None
    without include_stop); logprob = their sum (member_logprob without a stop term); node_logprobs fp32 [P, N + 1] per trie node
    (column 0, the root, is 0); n_members [P]; rows_evaluated: the decoder rows the call ran through the layers, all passes.
    With per-row tries M and N are the maxima: -inf (node_logprobs: 0) beyond a row's own count."""

    def __init__(self, member_logprob, stop_logprob, node_logprobs, n_members, rows_evaluated: int):
        self.member_logprob, self.stop_logprob, self.node_logprobs = member_logprob, stop_logprob, node_logprobs
        self.n_members, self.rows_evaluated = n_members, int(rows_evaluated)
        self.logprob = member_logprob if stop_logprob is None else member_logprob + stop_logprob

    def topk(self, k: int):
        """(values, member indices), [P, k] each: descending, ties to the lower member index."""
        if k < 1 or k > self.logprob.shape[1]:
            raise ValueError(f"topk: k={k} for {self.logprob.shape[1]} members")
        vals, idx = torch.sort(self.logprob, dim=1, descending=True, stable=True)
        return vals[:, :k], idx[:, :k]


class TrieSearchResult:
    """What search_trie() returns.  member_index int64 [P, top]: indices into trie.member_ids / member_strings (per_row: of that
    row's trie), best first, -1 where fewer members were found; logprob fp32 [P, top] descending (-inf at -1) = member_logprob
    (+ stop_logprob with include_stop; None without) - TrieScores' definitions.  levels: levels run (the most of any group);
    rows_decoded: decoder rows run through the layers; exhaustive bool [P]: no candidate of the prompt ever went without a beam
    slot - the row is then score_trie(...).topk(top); n_members [P].  trace (return_trace=True): per group and level a dict of
    flat [prompts x num_beams] CPU tensors - prompt, the new beams' node / alive / edge_logprob / score, and the beams they came
    from: from_node / from_alive / from_stop (the stop term of a beam on a member node, -inf otherwise)."""

    def __init__(self, member_index, member_logprob, stop_logprob, levels: int, rows_decoded: int, exhaustive, n_members, trace=None):
        self.member_index, self.member_logprob, self.stop_logprob = member_index, member_logprob, stop_logprob
        self.logprob = member_logprob if stop_logprob is None else member_logprob + stop_logprob
        self.levels, self.rows_decoded, self.exhaustive, self.n_members, self.trace = int(levels), int(rows_decoded), exhaustive, n_members, trace


# capacities of the processor kernel (include/opus_pllm.h, opus_set_logits_processors)
LP_MAX_BAD, LP_MAX_BAD_LEN, LP_MAX_BAD_IDS = 256, 8, 1024


class LookupStats:
    """What a generate(prompt_lookup_num_tokens=k) call did: verify passes, plain decode steps, ids drafted (by unfinished rows,
    over all passes) and ids accepted (the lockstep a, summed over the passes)."""

    def __init__(self, passes: int = 0, plain_steps: int = 0, drafted: int = 0, accepted: int = 0):
        self.passes, self.plain_steps, self.drafted, self.accepted = passes, plain_steps, drafted, accepted

    def __repr__(self):
        return (f"LookupStats(passes={self.passes}, plain_steps={self.plain_steps}, drafted={self.drafted}, "
                f"accepted={self.accepted})")


LOOKUP_MAX_NGRAM = 8           # csrc/lookup.hip LK_MAX_NGRAM


def _check_lookup(k: int, max_ngram, B: int, max_batch: int, *, do_sample=False, num_beams=1, nret=1, guidance=None, prefix=None,
                  lproc=None, constraint=None, outputs=False) -> int:
    """The argument checks of generate(prompt_lookup_num_tokens=k); returns max_matching_ngram_size (default 2)."""
    if k < 0:
        raise ValueError(f"`prompt_lookup_num_tokens` has to be a positive integer (got {k})")
    m = 2 if max_ngram is None else int(max_ngram)
    if not 1 <= m <= LOOKUP_MAX_NGRAM:
        raise ValueError(f"`max_matching_ngram_size` has to lie in [1, {LOOKUP_MAX_NGRAM}] (got {m})")
    why = "prompt_lookup_num_tokens is built for greedy search, where the verified ids are exactly those of plain generate(): "
    if do_sample:
        raise NotImplementedError(why + "do_sample=True needs speculative sampling, which is not built")
    if num_beams > 1:
        raise NotImplementedError(why + "num_beams > 1 would have to verify every beam's draft")
    if nret > 1:
        raise NotImplementedError(why + "num_return_sequences > 1 exists for sampling and beams only")
    if guidance is not None:
        raise NotImplementedError(why + "guidance_scale pairs every row with a negative row, whose pass rows are not built")
    if prefix is not None:
        raise NotImplementedError(why + "generate(prefix=...) starts from a detached cache, whose history the draft does not see")
    if lproc is not None:
        raise NotImplementedError(why + "the logits processors (repetition_penalty, no_repeat_ngram_size, bad_words_ids, "
                                        "min_length / min_new_tokens) would have to run on every position of a pass")
    if constraint is not None:
        raise NotImplementedError(why + "a TokenTrie's automaton would have to step through every position of a pass")
    if outputs:
        raise NotImplementedError(why + "output_scores / output_logits / output_token_logprobs are not collected from the passes")
    if B * (k + 1) > max_batch or B > 64:
        raise ValueError(f"prompt_lookup_num_tokens={k} verifies batch x (k + 1) = {B} x {k + 1} positions per pass: it needs a "
                         f"context with max_batch >= {B * (k + 1)} (this one holds max_batch={max_batch}) and at most 64 rows")
    return m


def lookup_history(input_ids, attention_mask=None, lookup_ids=None, n_prot_tokens: int = 1):
    """The rows' searchable histories for prompt-lookup drafts: (int32 array [B, L], lengths [B]).  Row b: its prompt ids without
    the padding, -1 at every position a protein block is spliced into, then - with lookup_ids ([B, L'] ids or a list of B id
    lists; negative ids are dropped) - one -1 and that corpus."""
    ids = np.asarray(input_ids.cpu() if hasattr(input_ids, "cpu") else input_ids).astype(np.int64)
    B = ids.shape[0]
    m = None if attention_mask is None else np.asarray(attention_mask.cpu() if hasattr(attention_mask, "cpu") else attention_mask).astype(bool)
    if lookup_ids is not None:
        if hasattr(lookup_ids, "cpu"):
            lookup_ids = lookup_ids.cpu().tolist()
        if len(lookup_ids) != B:
            raise ValueError(f"`lookup_ids` holds {len(lookup_ids)} rows, the batch {B}")
    rows = []
    for b in range(B):
        h = []
        for j in range(ids.shape[1]):
            if m is not None and not m[b, j]:
                continue
            t = int(ids[b, j])
            h.extend([-1] * n_prot_tokens if t == DEFAULT_SEQ_TOKEN_INDEX else [t])
        if lookup_ids is not None:
            corpus = [int(t) for t in lookup_ids[b] if int(t) >= 0]
            if corpus:
                h.append(-1)
                h.extend(corpus)
        rows.append(h)
    L = max(1, max(len(h) for h in rows))
    out = np.full((B, L), -1, dtype=np.int32)
    for b, h in enumerate(rows):
        out[b, :len(h)] = h
    return out, np.asarray([len(h) for h in rows], dtype=np.int32)


def _top_logprobs_arg(k, vocab: Optional[int]) -> int:
    """generate() / forward()'s top_logprobs: None -> 0 (off); an int in 1..min(20, vocabulary), else ValueError."""
    if k is None:
        return 0
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= TOP_LOGPROBS_MAX:
        raise ValueError(f"`top_logprobs` has to be an integer from 1 to {TOP_LOGPROBS_MAX} (got {k!r})")
    if vocab is not None and int(k) > vocab:
        raise ValueError(f"`top_logprobs` ({int(k)}) exceeds the vocabulary ({vocab})")
    return int(k)


def _guidance_scale(g) -> Optional[float]:
    """generate(guidance_scale=g): None when guidance is off (g None or 1, as in transformers), else the finite float."""
    if g is None:
        return None
    if isinstance(g, (bool, str)) or not isinstance(g, (int, float, np.integer, np.floating)) or not np.isfinite(float(g)):
        raise ValueError(f"`guidance_scale` has to be a finite number (got {g!r})")
    return None if float(g) == 1.0 else float(g)


def _left_pack(rows: List[List[int]]):
    """Lists of ids -> (ids int64 [P, T], mask bool [P, T]) on the CPU, left-padded with id 0 to the longest row."""
    T = max(len(r) for r in rows)
    ids = torch.zeros((len(rows), T), dtype=torch.int64)
    mask = torch.zeros((len(rows), T), dtype=torch.bool)
    for b, r in enumerate(rows):
        if r:
            ids[b, T - len(r):] = torch.tensor(r, dtype=torch.int64)
            mask[b, T - len(r):] = True
    return ids, mask


def protein_free_twin(input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None):
    """The default negative prompt of generate(guidance_scale=...): every row of the prompt with its masked-out positions and
    every <seq> placeholder dropped, left-padded to the longest row -> (ids int64 [P, Tn], mask bool [P, Tn]) on the CPU."""
    ids = input_ids.detach().to("cpu", torch.int64)
    m = torch.ones_like(ids, dtype=torch.bool) if attention_mask is None else attention_mask.detach().to("cpu").bool()
    if ids.ndim != 2 or m.shape != ids.shape:
        raise ValueError(f"input ids [P, T] and attention_mask of the same shape (got {tuple(ids.shape)} and {tuple(m.shape)})")
    rows = [[int(t) for t, k in zip(r.tolist(), mr.tolist()) if k and t != DEFAULT_SEQ_TOKEN_INDEX] for r, mr in zip(ids, m)]
    for b, r in enumerate(rows):
        if not r:
            raise ValueError(f"row {b} of the prompt holds nothing but <seq> placeholders: its protein-free twin is empty "
                             "(pass negative_prompt_ids)")
    return _left_pack(rows)


def _explicit_negative_prompt(neg_ids, neg_mask, P: int):
    """negative_prompt_ids / negative_prompt_attention_mask as given, checked: P rows, no <seq> placeholder, no empty row."""
    ids = torch.as_tensor(neg_ids).detach().to("cpu", torch.int64)
    if ids.ndim != 2 or ids.shape[0] != P:
        raise ValueError(f"`negative_prompt_ids` has to be [batch, Tn] with one row per prompt: got {tuple(ids.shape)} for "
                         f"{P} prompts")
    m = torch.ones_like(ids, dtype=torch.bool) if neg_mask is None else torch.as_tensor(neg_mask).detach().to("cpu").bool()
    if m.shape != ids.shape:
        raise ValueError(f"`negative_prompt_attention_mask` {tuple(m.shape)} does not match `negative_prompt_ids` {tuple(ids.shape)}")
    if bool(((ids == DEFAULT_SEQ_TOKEN_INDEX) & m).any()):
        raise ValueError("`negative_prompt_ids` may hold no <seq> placeholder: the negative rows are text only")
    if bool((m.sum(dim=1) == 0).any()):
        raise ValueError("`negative_prompt_ids` has an empty row")
    return ids, m


def spliced_length(input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], n_prot_tokens: int, max_length: int = 0) -> int:
    """Positions the longest row takes after the splice: its unmasked ids, every <seq> placeholder standing for n_prot_tokens
    (cut at max_length when > 0, as the splice does)."""
    ids = input_ids.detach().to("cpu", torch.int64)
    m = torch.ones_like(ids, dtype=torch.bool) if attention_mask is None else attention_mask.detach().to("cpu").bool()
    n = m.sum(dim=1) + (n_prot_tokens - 1) * ((ids == DEFAULT_SEQ_TOKEN_INDEX) & m).sum(dim=1)
    T = int(n.max())
    return min(T, max_length) if max_length > 0 else T


def pad_left_common(a: torch.Tensor, a_mask: torch.Tensor, b: torch.Tensor, b_mask: torch.Tensor, fill=0):
    """Two left-padded sets [P, Ta, ...] and [P, Tb, ...] with masks [P, Ta] / [P, Tb] -> one set [2 P, T, ...] and its mask
    [2 P, T], T = max(Ta, Tb): the rows of `a`, then those of `b`, each moved to the right end, `fill` and mask 0 in front."""
    T = max(a.shape[1], b.shape[1])
    P = a.shape[0]
    out = torch.full((P + b.shape[0], T) + tuple(a.shape[2:]), fill, dtype=a.dtype, device=a.device)
    mask = torch.zeros((P + b.shape[0], T), dtype=a_mask.dtype, device=a_mask.device)
    out[:P, T - a.shape[1]:] = a
    out[P:, T - b.shape[1]:] = b.to(a.dtype)
    mask[:P, T - a.shape[1]:] = a_mask
    mask[P:, T - b.shape[1]:] = b_mask.to(a_mask.dtype)
    return out, mask


_WARPER_NAMES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
_WARPERS_OFF = (0.0, 1.0, 0.0, 0.0)


def _sampling_warpers(kwargs: dict):
    """Pops generate()'s truncation warpers from kwargs and checks them with transformers' messages (ValueError).  Returns None when
    all are off, else (min_p, typical_p, epsilon_cutoff, eta_cutoff) with the off value in an unused place.  Off: min_p None / 0,
    typical_p None / 1.0, epsilon_cutoff and eta_cutoff None / 0 (transformers' defaults)."""
    vals = [kwargs.pop(k, None) for k in _WARPER_NAMES]
    for name, v in zip(_WARPER_NAMES, vals):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer))):
            raise ValueError(f"`{name}` has to be a float, but is {v!r}")
    min_p, typical, eps, eta = (None if v is None else float(v) for v in vals)
    if min_p is not None and not 0.0 <= min_p <= 1.0:
        raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
    if typical is not None and typical != 1.0 and not 0.0 < typical < 1.0:
        raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {typical}")
    for name, v in (("epsilon_cutoff", eps), ("eta_cutoff", eta)):
        if v is not None and v != 0.0 and not 0.0 < v < 1.0:
            raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
    out = (min_p or 0.0, 1.0 if typical is None else typical, eps or 0.0, eta or 0.0)
    return None if out == _WARPERS_OFF else out


def _logits_processors(kwargs: dict, eos: Sequence[int], vocab: Optional[int]):
    """Pops generate()'s logits-processor options from kwargs and checks them as transformers does (ValueError), plus the
    kernel's capacities.  Returns None when every option is off, else (repetition_penalty, no_repeat_ngram_size,
    min_new_tokens or None, min_length or None, bad_words_ids as a tuple of tuples).  Off: repetition_penalty None / 1.0,
    no_repeat_ngram_size None / 0 (transformers' defaults), no bad words, min_length / min_new_tokens None / 0 - and both are
    no-ops without EOS ids (transformers builds no processor then).  min_new_tokens wins over min_length."""
    pen = kwargs.pop("repetition_penalty", None)
    ngram = kwargs.pop("no_repeat_ngram_size", None)
    bad = kwargs.pop("bad_words_ids", None)
    min_new = kwargs.pop("min_new_tokens", None)
    min_len = kwargs.pop("min_length", None)
    if pen is not None:
        if isinstance(pen, bool) or not isinstance(pen, (int, float)) or not float(pen) > 0 or float(pen) == float("inf"):
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {pen}")
        pen = float(pen)
    if ngram is not None:
        if isinstance(ngram, bool) or not isinstance(ngram, (int, np.integer)) or ngram < 0:
            raise ValueError(f"`no_repeat_ngram_size` has to be a strictly positive integer, but is {ngram}")
        ngram = int(ngram)
    for name, v in (("min_new_tokens", min_new), ("min_length", min_len)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0):
            raise ValueError(f"`{name}` has to be a non-negative integer, but is {v}")
    if bad is not None:
        if not isinstance(bad, (list, tuple)) or len(bad) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad}.")
        if any(not isinstance(w, (list, tuple)) or len(w) == 0 for w in bad):
            raise ValueError(f"`bad_words_ids` has to be a list of non-empty lists, but is {bad}.")
        for w in bad:
            for t in w:
                if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0 or (vocab is not None and t >= vocab):
                    raise ValueError(f"`bad_words_ids` holds ids in [0, {vocab if vocab is not None else 'V'}), but is {bad}.")
        if len(bad) > LP_MAX_BAD:
            raise ValueError(f"`bad_words_ids` has {len(bad)} entries: at most {LP_MAX_BAD} are built")
        if max(len(w) for w in bad) > LP_MAX_BAD_LEN:
            raise ValueError(f"a `bad_words_ids` entry has {max(len(w) for w in bad)} ids: at most {LP_MAX_BAD_LEN} are built")
        if sum(len(w) for w in bad) > LP_MAX_BAD_IDS:
            raise ValueError(f"`bad_words_ids` holds {sum(len(w) for w in bad)} ids: at most {LP_MAX_BAD_IDS} in all are built")
        bad = tuple(tuple(int(t) for t in w) for w in bad)
    if not eos:
        min_new = min_len = None
    if (pen is None or pen == 1.0) and not ngram and bad is None and not min_new and not min_len:
        return None
    return (1.0 if pen is None else pen, ngram or 0, min_new, min_len, bad or ())


def counted_tokens(ids: torch.Tensor, eos: Sequence[int], stop: Sequence[int] = ()) -> torch.Tensor:
    """Positions of each row of new ids [B, n] up to and including the token that finished it - an EOS id, or the last id of the
    stop sequence - or all n (int64 [B], on the device of `ids`): the positions generate()'s token_logprobs count."""
    B, n = ids.shape
    if n == 0:
        return torch.zeros(B, dtype=torch.int64, device=ids.device)
    done = torch.zeros((B, n), dtype=torch.bool, device=ids.device)
    if len(eos):
        done |= torch.isin(ids, torch.tensor(list(eos), dtype=ids.dtype, device=ids.device))
    k = len(stop)
    if k and n >= k:
        win = ids.unfold(1, k, 1)                                       # [B, n - k + 1, k]: ids t - k + 1 .. t
        done[:, k - 1:] |= (win == torch.tensor(list(stop), dtype=ids.dtype, device=ids.device)).all(-1)
    pos = torch.arange(1, n + 1, device=ids.device).expand(B, n)
    return torch.where(done, pos, torch.full_like(pos, n)).min(dim=1).values


class _FieldsOutput:
    """Indexed like transformers' ModelOutput: attributes and keys are the fields in `_fields`; keys(), integer indices,
    iteration and to_tuple() run over the fields that are not None.  Other attributes are extensions (attributes only)."""
    _fields: tuple = ()

    def keys(self):
        return [k for k in self._fields if getattr(self, k) is not None]

    def to_tuple(self):
        return tuple(getattr(self, k) for k in self.keys())

    def __getitem__(self, k):
        if isinstance(k, str):
            if k not in self.keys():
                raise KeyError(k)
            return getattr(self, k)
        return self.to_tuple()[k]

    def __contains__(self, k):
        return k in self.keys()

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())


class GenerateDecoderOnlyOutput(_FieldsOutput):
    """generate(return_dict_in_generate=True) for greedy and sampling, as transformers' class of that name: `sequences` (the
    new ids [B, n]), `scores` / `logits` (tuples of n fp32 [B, V] tensors, or None); `attentions`, `hidden_states` and
    `past_key_values` stay None.  Extension fields (output_token_logprobs=True; attributes only): `token_logprobs` fp32 [B, n],
    `logprob` fp32 [B], `n_tokens` [B]."""
    _fields = ("sequences", "scores", "logits", "attentions", "hidden_states", "past_key_values")

    def __init__(self, sequences=None, scores=None, logits=None, attentions=None, hidden_states=None, past_key_values=None,
                 token_logprobs=None, logprob=None, n_tokens=None):
        self.sequences, self.scores, self.logits = sequences, scores, logits
        self.attentions, self.hidden_states, self.past_key_values = attentions, hidden_states, past_key_values
        self.token_logprobs, self.logprob, self.n_tokens = token_logprobs, logprob, n_tokens
        self.prefix = None               # return_prefix=True (extension; attribute only): the detached OpusPrefix of prompt + answer


class GenerateBeamDecoderOnlyOutput(_FieldsOutput):
    """generate(return_dict_in_generate=True, num_beams > 1), as transformers' class of that name: `sequences` (the best
    hypothesis of every row, new ids [B, n]) and `sequences_scores` fp32 [B] (its length-normalised log-probability, the value
    last_beam_scores holds); the per-step fields stay None."""
    _fields = ("sequences", "sequences_scores", "scores", "logits", "beam_indices", "attentions", "hidden_states",
               "past_key_values")

    def __init__(self, sequences=None, sequences_scores=None, scores=None, logits=None, beam_indices=None, attentions=None,
                 hidden_states=None, past_key_values=None):
        self.sequences, self.sequences_scores, self.scores, self.logits = sequences, sequences_scores, scores, logits
        self.beam_indices, self.attentions, self.hidden_states, self.past_key_values = (beam_indices, attentions, hidden_states,
                                                                                         past_key_values)


class CausalLMOutput:
    """What forward() returns, indexed like transformers' CausalLMOutputWithPast: attributes and keys `loss`, `logits`,
    `past_key_values` (always None here); integer indices / to_tuple() run over the fields that are not None.  Extension fields
    (attributes only): `token_logprobs` fp32 [B, T] and `n_tokens`."""
    _fields = ("loss", "logits", "past_key_values")

    def __init__(self, loss=None, logits=None, past_key_values=None, token_logprobs=None, n_tokens=0):
        self.loss, self.logits, self.past_key_values = loss, logits, past_key_values
        self.token_logprobs, self.n_tokens = token_logprobs, n_tokens

    def keys(self):
        return [k for k in self._fields if getattr(self, k) is not None]

    def to_tuple(self):
        return tuple(getattr(self, k) for k in self.keys())

    def __getitem__(self, k):
        if isinstance(k, str):
            if k not in self.keys():
                raise KeyError(k)
            return getattr(self, k)
        return self.to_tuple()[k]

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())
