"""generate_continuous() on the GPU: the refill launches alone (bit for bit, on a poisoned cache), the numerics of a refilled row
against the plain prefill of the longer prompt, the whole call against plain generate() batches, the stop sequence across a
refill boundary, sampling, and the context afterwards.  Observed figures go through gpu_helpers.record (those of the MI355X run are
committed as profiles/continuous_parity.jsonl)."""
import ctypes as C

import numpy as np
import pytest
import torch

import opus_pllm_amd as opa
from opus_pllm_amd import _cabi, continuous as cont
import continuous_checks as cc
import forward_checks as fc
import prefix_generate_checks as pg
from gpu_helpers import record, rel_l2

pytestmark = pytest.mark.gpu

PAD = cc.PAD
DECODE_VS_PREFILL = 1.5e-2     # rel-L2, "decode step vs prefill of the longer prompt" on micro fixtures (tests/test_gpu_parity.py REL_L2)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ the C entries, driven directly
class Session:
    """One opus_stream_* session on text-only rows."""

    def __init__(self, model, rows, max_new, eos=()):
        self.m, self.B = model, len(rows)
        ids, mask = pg.left_pad(rows)
        emb, m = pg.embed(model, ids, mask, left=True)
        emb, m = emb.contiguous(), m.to(torch.uint8).contiguous()
        self.T0 = int(ids.shape[1])
        cfg = model.cfg
        eos_arr = (C.c_int32 * max(1, len(eos)))(*eos)
        s = model._enter()
        with torch.cuda.stream(model._stream):
            self.ids = torch.full((cfg.max_batch, cfg.max_new_tokens), PAD, dtype=torch.int32, device=model.device)
            _cabi.check(model._lib.opus_stream_begin(model._ctx, emb.data_ptr(), m.data_ptr(), self.B, self.T0, max_new, eos_arr, len(eos),
                                                     PAD, 0.0, 1.0, 0, self.ids.data_ptr(), s))
        model._leave()

    def run_to(self, t):
        t_out, h_end = C.c_int32(0), (C.c_int32 * self.B)()
        _cabi.check(self.m._lib.opus_stream_run(self.m._ctx, t, self.B + 1, t, C.byref(t_out), h_end, self.m._stream.cuda_stream))
        assert t_out.value == t
        return list(h_end)

    def state(self, poison=0):
        a = [(C.c_int32 * self.B)() for _ in range(4)]
        epoch = C.c_int64(0)
        _cabi.check(self.m._lib.opus_debug_stream_state(self.m._ctx, a[0], a[1], a[2], a[3], C.byref(epoch), poison, self.m._stream.cuda_stream))
        return dict(kstart=list(a[0]), fin=list(a[1]), start=list(a[2]), end=list(a[3]), epoch=epoch.value)

    def snapshot(self, poison=0):
        st = self.state(poison)
        cfg = self.m.cfg
        k, v, _ = self.m.export_cache(st["epoch"], cfg.max_batch, cfg.max_prompt + cfg.max_new_tokens)
        st.update(k=k, v=v, logits=self.m.last_logits(self.B).clone(), ids=self.ids.clone())
        torch.cuda.synchronize()
        return st

    def refill(self, prefix, rows, src, lens):
        n = len(rows)
        snap = prefix._snap()
        s = self.m._enter()
        _cabi.check(self.m._lib.opus_stream_refill(self.m._ctx, C.byref(snap), n, (C.c_int32 * n)(*rows), (C.c_int32 * n)(*src),
                                                   prefix.last_logits.data_ptr(), (C.c_int32 * n)(*lens), s))
        self.m._leave()

    def end(self):
        h_end = (C.c_int32 * self.B)()
        s = self.m._enter()
        _cabi.check(self.m._lib.opus_stream_end(self.m._ctx, h_end, s))
        self.m._leave()
        return list(h_end)


def _rows(cfg, lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(3, cfg.dec_vocab, int(n)) for n in lens]


# (t, new prompts' lengths, L - len of the first listed row): one row per launch covers len x (L - len); three rows per launch
# take the snapshot rows in permuted order.  t = 0: straight behind the prefill; t > 0: rows that are done, id columns to clear.
REFILL_ONE = [(t, (n,), off) for n in (1, 31, 32, 33) for off, t in ((0, 0), (7, 3), (33, 10))]
REFILL_THREE = [(10, (31, 32, 33), 33), (3, (1, 33, 32), 32), (9, (31, 1, 33), 7)]


@pytest.mark.parametrize("hd,nh,nkv", [(16, 4, 2), (16, 4, 4), (64, 4, 2), (64, 2, 2)])
def test_refill_launches_alone_bit_for_bit(dev, hd, nh, nkv):
    """kv_place_kernel + stream_refill_kernel on a poisoned cache: slots [L - len, L) of the listed rows equal the snapshot, the
    rows' logits, kstart, start, fin, end and id columns t - 8 .. t - 1 are the new occupant's, and every other bit - the other
    slots, the other rows, their logits, kstart, fin and ids - is unchanged."""
    cfg = opa.micro(dec_dim=max(64, nh * hd), dec_heads=nh, dec_kv_heads=nkv, dec_head_dim=hd, max_prompt=72, max_batch=5,
                    max_new_tokens=24)
    model = fc.make_model(cfg, dev)
    helper = model.new_context()
    obs = {}
    for ci, (t, lens, off) in enumerate(REFILL_ONE + REFILL_THREE):
        L = lens[0] + off
        T0 = L - t
        assert T0 >= 1 and all(n <= L for n in lens)
        B = 5
        first = _rows(cfg, [T0, max(1, T0 - 3), 1, max(1, T0 // 2), T0], 50 + ci)
        eos = []
        if t:                                    # rows that are done at the boundary: row 0's second id as the EOS id
            probe = Session(model, first, max_new=12)
            probe.run_to(2)
            torch.cuda.synchronize()
            eos = [int(probe.ids[0, 1])]
            probe.end()
        sess = Session(model, first, max_new=12, eos=eos)
        assert sess.T0 == T0
        sess.run_to(t)
        before = sess.snapshot(poison=0x5B)
        if t:
            assert before["fin"][0] == 1 and 0 <= before["end"][0] <= 1 and 0 < sum(before["fin"]) < B, before["fin"]
        new = _rows(cfg, lens, 70 + ci)
        order = list(range(len(lens)))[::-1]                                       # snapshot row of listed row i
        pids, pmask = pg.left_pad([new[i] for i in np.argsort(order)])
        prefix = helper.cache_prefix(pids, attention_mask=pmask, detach=True, last_logits=True)
        rows = [3, 0, 4][: len(lens)] if len(lens) > 1 else [2]
        src = order
        snap_len = [int(x) for x in prefix.lengths.tolist()]
        assert [snap_len[p] for p in src] == list(lens)
        sess.refill(prefix, rows, src, list(lens))
        after = sess.snapshot()
        Tp = prefix.slots
        ek, ev, el, ei = before["k"].clone(), before["v"].clone(), before["logits"].clone(), before["ids"].clone()
        eks, efin, est, een = list(before["kstart"]), list(before["fin"]), list(before["start"]), list(before["end"])
        for r, p, n in zip(rows, src, lens):
            ek[:, r, :, L - n: L] = prefix._k[:, p, :, Tp - n:]
            ev[:, r, :, L - n: L] = prefix._v[:, p, :, Tp - n:]
            el[r] = prefix.last_logits[p]
            ei[r, max(0, t - 8): t] = -1
            eks[r], efin[r], est[r], een[r] = L - n, 0, t, -1
        o = dict(k=pg.same(after["k"], ek), v=pg.same(after["v"], ev), logits=pg.same(after["logits"], el),
                 ids=bool(torch.equal(after["ids"], ei)), kstart=after["kstart"] == eks, fin=after["fin"] == efin,
                 start=after["start"] == est, end=after["end"] == een,
                 placed_differs=not pg.same(after["k"], before["k"]))
        obs[f"t{t}_len{'_'.join(map(str, lens))}_off{off}"] = o
        sess.end()
    record(f"continuous.refill.hd{hd}_nh{nh}_kv{nkv}", obs)
    assert len(obs) == 15 and all(all(o.values()) for o in obs.values()), obs


def test_refilled_row_numerics_and_untouched_rows(dev):
    """After a refill, 3 steps: the refilled row's logits against prefill_logits (another context) of its prompt extended by the
    ids it emitted; the other rows bit-identical to the same session without the refill."""
    cfg = opa.micro(max_new_tokens=24)
    model = fc.make_model(cfg, dev)
    other = model.new_context()
    first = _rows(cfg, [14, 9, 5, 11], 3)
    new = _rows(cfg, [17], 4)[0]
    runs = {}
    for with_refill in (True, False):
        sess = Session(model, first, max_new=12)
        sess.run_to(5)
        if with_refill:
            pids, pmask = pg.left_pad([new])
            prefix = other.cache_prefix(pids, attention_mask=pmask, detach=True, last_logits=True)
            sess.refill(prefix, [1], [0], [17])
        lg = []
        for k in range(3):
            sess.run_to(6 + k)
            lg.append(model.last_logits(4).clone())
        torch.cuda.synchronize()
        runs[with_refill] = (lg, sess.ids[:4, :8].cpu().clone())
        sess.end()
    (lg_r, ids_r), (lg_p, ids_p) = runs[True], runs[False]
    rel, norms, vs_old = [], [], []
    for k in range(3):
        row = np.concatenate([new, ids_r[1, 5: 6 + k].numpy()])
        emb, m = pg.embed(other, *pg.left_pad([row]), left=True)
        ref = other.prefill_logits(emb, m)[0]
        rel.append(rel_l2(lg_r[k][1], ref))
        norms.append(float(ref.norm()))
        vs_old.append(rel_l2(lg_r[k][1], lg_p[k][1]))            # (the row's previous occupant, at the same steps)
    keep = [0, 2, 3]
    same = all(pg.same(lg_r[k][keep], lg_p[k][keep]) for k in range(3)) and bool(torch.equal(ids_r[keep], ids_p[keep]))
    record("continuous.refilled_row", dict(rel_l2=rel, ref_norm=norms, vs_previous_occupant=vs_old, other_rows_bitwise=same))
    assert min(norms) > 0 and min(vs_old) > 10 * DECODE_VS_PREFILL, (norms, vs_old)     # the comparison is not vacuous
    assert ids_r[1, 2:5].tolist() == [-1, -1, -1] and bool((ids_r[1, 5:8] >= 0).all())
    assert max(rel) < DECODE_VS_PREFILL, rel
    assert same


# ------------------------------------------------------------------------------------------------ the public call
def _plain_batches(model, prompts, seqs, eos, max_new, slots):
    """Plain generate() on batches of `slots`: (ids [N, max_new] padded, margins [N, max_new], counted lengths)."""
    rows, marg = [], []
    for b0 in range(0, len(prompts), slots):
        ids, mask = cc.left_pad([p.tolist() for p in prompts[b0: b0 + slots]])
        o = model.generate(ids, None if seqs is None else seqs[b0: b0 + slots], attention_mask=mask, pad_token_id=PAD,
                           eos_token_id=list(eos), max_new_tokens=max_new, return_dict_in_generate=True, output_logits=True)
        n = o.sequences.shape[1]
        r = torch.full((ids.shape[0], max_new), PAD, dtype=torch.long)
        r[:, :n] = o.sequences.cpu()
        m = torch.full((ids.shape[0], max_new), float("inf"))
        m[:, :n] = cc.margins_of(o.logits)
        rows.append(r)
        marg.append(m)
    rows, marg = torch.cat(rows), torch.cat(marg)
    return rows, marg, cc.lengths_under(rows.numpy(), tuple(eos))


@pytest.mark.parametrize("preset", ["micro_opt", "micro_qwen"])
def test_end_to_end_greedy(dev, preset):
    seed, decisive = cc.E2E_SEEDS[preset]
    cfg = getattr(opa, preset)(max_batch=cc.E2E_SLOTS, max_prompt=cc.E2E_MAX_PROMPT, max_new_tokens=cc.E2E_S)
    model = fc.make_model(cfg, dev)
    prompts, seqs = cc.e2e_prompts(cfg, seed)
    lens = [len(p) - 1 + cfg.n_prot_tokens for p in prompts]
    assert max(lens) - min(lens) >= 40 and max(lens[4:]) > max(lens[:4])
    free, _, _ = _plain_batches(model, prompts, seqs, (), cc.E2E_MAX_NEW, cc.E2E_SLOTS)
    eos = cc.choose_eos(free.numpy())
    ref, marg, ref_len = _plain_batches(model, prompts, seqs, eos, cc.E2E_MAX_NEW, cc.E2E_SLOTS)
    assert len(set(ref_len)) >= 4, ref_len
    out = model.generate_continuous(prompts, seqs, max_new_tokens=cc.E2E_MAX_NEW, eos_token_id=eos, pad_token_id=PAD, slots=cc.E2E_SLOTS,
                                    return_dict_in_generate=True)
    frac, ids_ok, len_ok = cc.decisive_compare(out.sequences, ref, marg, ref_len)
    sim, _ = cont.simulate(lens, [int(n) for n in out.n_tokens], cc.E2E_SLOTS, cc.E2E_MAX_NEW, cc.E2E_S)
    sim.pop("placements")
    record(f"continuous.e2e.{preset}", dict(decisive=frac, ids_equal=ids_ok, lengths_equal=len_ok, eos=eos, lengths=ref_len,
                                            smallest_margin=float(min(float(marg[p, :n].min()) for p, n in enumerate(ref_len))),
                                            stats=out.stats))
    assert all(s.dtype == torch.long and s.ndim == 1 for s in out.sequences) and len(out.sequences) == 11
    assert frac == decisive, (frac, marg)
    assert ids_ok and len_ok, (out.sequences, ref, ref_len)
    assert out.n_tokens.tolist() == [len(s) for s in out.sequences]
    st = out.stats
    assert st["rows_refilled"] == 11 - cc.E2E_SLOTS and st["live_row_steps"] == sum(len(s) for s in out.sequences)
    assert st["sessions"] >= 2 and st["slot_steps"] >= st["live_row_steps"]
    assert st == sim, (st, sim)                           # the device ran the schedule the pure function plans
    assert model.stat("stream_steps") == st["decode_steps"] and model.stat("stream_refills") == st["refills"]
    again = model.generate_continuous(prompts, seqs, max_new_tokens=cc.E2E_MAX_NEW, eos_token_id=eos, pad_token_id=PAD, slots=cc.E2E_SLOTS)
    assert all(torch.equal(a, b) for a, b in zip(again, out.sequences))


def test_stop_sequence_across_a_refill_boundary(dev):
    """One decode row, two prompts: the row's first occupant ends on its budget and emits pad ids until the refill; the stop
    sequence [pad, first id of the second answer] is completed only by the second occupant's first id TOGETHER with that tail.
    The refill clears the tail, so the second answer must not stop."""
    cfg = opa.micro(max_new_tokens=32)
    model = fc.make_model(cfg, dev)
    prompts = [torch.from_numpy(r) for r in _rows(cfg, [9, 7], 11)]
    kw = dict(max_new_tokens=4, pad_token_id=PAD, slots=1, return_dict_in_generate=True)
    free = model.generate_continuous(prompts, None, **kw)
    assert free.stats["sessions"] == 1 and free.stats["rows_refilled"] == 1 and [len(s) for s in free.sequences] == [4, 4]
    b = free.sequences[1].tolist()
    assert PAD not in b and PAD not in free.sequences[0].tolist()
    out = model.generate_continuous(prompts, None, stop_sequence=[PAD, b[0]], **kw)
    model.set_stop_sequence(None)
    record("continuous.stop_across_refill", dict(free=[s.tolist() for s in free.sequences], stopped=[s.tolist() for s in out.sequences]))
    assert out.sequences[1].tolist() == b and out.sequences[0].tolist() == free.sequences[0].tolist()
    # and a stop sequence inside one answer still ends it there
    cut = model.generate_continuous(prompts, None, stop_sequence=b[1:3], **kw)
    model.set_stop_sequence(None)
    assert cut.sequences[1].tolist() == b[:3]


def test_sampling_reproduces_itself_and_stays_in_the_kept_set(dev):
    cfg = opa.micro(max_new_tokens=32)
    model = fc.make_model(cfg, dev)
    other = model.new_context()
    rows = _rows(cfg, [9, 14, 5, 11, 7, 16, 6], 21)
    prompts = [torch.from_numpy(r) for r in rows]
    kw = dict(max_new_tokens=6, pad_token_id=PAD, slots=3, do_sample=True, temperature=1.0, top_k=2, seed=5)
    a = model.generate_continuous(prompts, None, **kw)
    b = model.generate_continuous(prompts, None, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(len(x) == 6 for x in a)
    c = model.generate_continuous(prompts, None, **dict(kw, seed=6))
    assert any(not torch.equal(x, y) for x, y in zip(a, c))
    # the plain path's kept set, teacher-forced: prefill_logits of prompt + the ids drawn so far; an id is admissible when its logit
    # reaches the second largest one (to within the decisive-step margin, as the two paths' logits differ in the last bits)
    strict = loose = 0
    for k in range(6):
        for g0 in range(0, len(rows), cfg.max_batch):
            grp = list(range(g0, min(g0 + cfg.max_batch, len(rows))))
            emb, m = pg.embed(other, *pg.left_pad([np.concatenate([rows[p], a[p][:k].numpy()]) for p in grp]), left=True)
            lg = other.prefill_logits(emb, m).float().cpu()
            for i, p in enumerate(grp):
                second = torch.topk(lg[i], 2).values[1]
                got = lg[i, int(a[p][k])]
                strict += int(got >= second)
                loose += int(got >= second - cc.MARGIN_TAU)
    record("continuous.sampling", dict(draws=6 * len(rows), in_top2=strict, in_top2_within_margin=loose))
    assert loose == 6 * len(rows), (strict, loose)
    model._set_top_k(model.default_top_k)


def test_the_context_afterwards(dev):
    cfg = opa.micro(max_new_tokens=32)
    model = fc.make_model(cfg, dev)
    rows = _rows(cfg, [9, 14, 5, 11, 7], 31)
    ids, mask = pg.left_pad(rows)
    before = model.generate(ids, attention_mask=mask, pad_token_id=PAD, max_new_tokens=6)
    live = model.cache_prefix(ids, attention_mask=mask)
    cached = model.stat("graphs_cached")
    out = model.generate_continuous([torch.from_numpy(r) for r in rows], None, max_new_tokens=6, pad_token_id=PAD, slots=2)
    assert len(out) == 5 and model.stat("stream_graph") == 1 and model.stat("graphs_cached") == cached
    with pytest.raises(_cabi.OpusError) as e:
        model.export_cache(live._epoch, 5, int(ids.shape[1]))
    assert e.value.code == -6
    with pytest.raises(_cabi.OpusError) as e:
        model.score_continuations(live, [torch.tensor([5, 6])] * 5)
    assert e.value.code == -6
    assert model.decode_logits(torch.tensor([5, 6], device=dev)).shape == (2, cfg.dec_vocab)     # a decode step is legal
    after = model.generate(ids, attention_mask=mask, pad_token_id=PAD, max_new_tokens=6)
    assert torch.equal(before, after)
    # capacity: the native entry refuses what the Python call checks first
    with pytest.raises(_cabi.OpusError) as e:
        Session(model, rows, max_new=cfg.max_new_tokens + 1)
    assert e.value.code == -2


def test_eval_loop_continuous_saves_what_the_batched_loop_saves():
    """eval_ddp.annotate_continuous (--continuous) on the synthetic tokenizer against annotate(): the same [n, max_new] id matrix on
    the steps the batched run's own logits decide."""
    import importlib.util
    import os
    from opus_pllm_amd import builder, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_ddp", os.path.join(root, "opus-pllm_amd", "eval_ddp.py"))
    ddp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ddp)
    tok, model, _ = builder.load_pretrained_model("synthetic:c1_tiny", "synthetic", "c1_tiny", device="cuda:0", max_batch=4,
                                                  max_enc_tokens=258, max_prompt=64, max_new_tokens=32)
    items = [dict(instruction=f"What is the function of protein {i}?", input=synth.synth_protein(20 + 11 * (i % 9), i), output="x")
             for i in range(7)]
    orig, logits = model.generate, []

    def spy(*a, **k):                                  # the batched run's per-step logits, for its own margins
        out = orig(*a, **dict(k, return_dict_in_generate=True, output_logits=True))
        logits.append(out.logits)
        return out.sequences
    model.generate = spy
    plain = ddp.annotate(model, tok, items, "", 4, 8, temperature=0.0, inflight=1)
    model.generate = orig
    stats = {}
    got = ddp.annotate_continuous(model, tok, items, "", 8, slots=4, stats_out=stats)
    assert got.shape == plain.shape == (7, 8) and stats["rows_refilled"] == 3 and stats["live_row_steps"] <= stats["slot_steps"]
    at, obs = 0, []
    for lg in logits:
        n, w = lg[0].shape[0], len(lg)
        obs.append(pg.decisive_compare(got[at: at + n, :w], plain[at: at + n, :w], lg))
        at += n
    record("continuous.driver", dict(batches=obs, stats=stats))
    assert at == 7 and all(b["ids_equal"] for b in obs), (obs, got, plain)
