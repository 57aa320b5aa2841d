"""Grammar-constrained decoding on the GPU: the device state machine alone (`mrmt3_grammar_advance`) and inside the
captured step (`dec_grammar_step` behind the greedy, sampled and beam tails), against the host restatement tests/grammar_ref.py.

  (5) kernel exact: every step's mask and the final `active` sets equal the host's, bit for bit, reparenting included;
  (6) decode exact: every emitted token is what the tail's rule gives on the device's own copied logits under the host's mask
      for that row's history (greedy: argmax; sampled: tests/sample_ref.py; beam: tests/beam_ref.py under a mask per row);
  (7) the property: constrained output decodes with 0 invalid and 0 dropped events, unconstrained output of the same
      near-noise golden models does not;
  (8) chains: a whole song of a segment-memory model decodes with 0 invalid events end to end (the first segment starts
      from the empty carry, the next from what the one before left sounding);
  (9) plumbing: log-probabilities over the allowed set, the prefix decode, on -> off -> on, off = the parent's behaviour,
      InferenceHandler.
Helpers are copies of tests/test_sample_gpu.py's (not imported)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grammar_ref as gr  # noqa: E402
import sample_ref as R  # noqa: E402
from contrib import metrics_utils, note_sequences, vocabularies  # noqa: E402

pytestmark = pytest.mark.gpu

LOGP_TOL = 2e-5            # as tests/test_sample_gpu.py: f32 log-softmax of these rows against fp64
B9, STEPS = 9, 96          # 9 rows: not a multiple of the 8 rows per workgroup
CODEC = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(variant, dtype, dev):
    from mrmt3.synthetic import T5_SMALL
    if variant == "t5":
        from models.t5 import T5ForConditionalGeneration
        m = T5ForConditionalGeneration(T5_SMALL, compute_dtype=dtype)
    elif variant == "segmem_v1":
        from models.t5_segmem import T5SegMem
        m = T5SegMem(T5_SMALL, segmem_num_layers=1, segmem_length=64, compute_dtype=dtype)
    else:
        from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev
        m = T5SegMemV2WithPrev(T5_SMALL, segmem_num_layers=1, segmem_length=64, compute_dtype=dtype)
    m = m.load_golden().to(dev).eval()
    m.engine.prepare(False)
    return m


def _enc(m, B, seed, frames=256):
    from mrmt3.synthetic import synth_mel
    mel = torch.from_numpy(synth_mel(B, frames=frames, seed=seed)).to(m.device)
    with torch.no_grad():
        return mel, m.engine.encode(mel).view(B, frames, m.cfg["d_model"])


def _grammar(**kw):
    from mrmt3.grammar import EventGrammar
    return EventGrammar.from_codec(CODEC, **kw)


def _carry_bits(carries, dev):
    return torch.from_numpy(np.stack([gr.set_to_bits(c) for c in carries])).to(dev)


# ---- (5) the kernel alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1536, 1491])          # the model's head; the codec's own size (rows of the mask not 4-byte aligned)
def test_advance_kernel_matches_the_host_bit_for_bit(dev, V):
    from mrmt3 import lib
    rows, steps = B9, 300
    rs = np.random.RandomState(5)
    ban = [1135 + 7, 1004 + 60]
    ban_dev = torch.zeros(V, dtype=torch.uint8)
    ban_dev[ban] = 1
    ban_dev = ban_dev.to(dev)
    for reparent in (False, True):
        # pass 1: every row walks alone, a carry on the odd rows, rows that draw EOS idle on pad afterwards.
        # pass 2: rows swap histories at random (all rows of a beam group share one carry); EOS is not drawn.
        shared = gr.random_carry(rs)
        carries = [shared if reparent else (gr.random_carry(rs) if r % 2 else None) for r in range(rows)]
        use_ban = ban if reparent else None
        refs = [gr.GrammarRef(CODEC, V=V, carry=c, ban=use_ban) for c in carries]
        want = [np.stack([g.allowed() for g in refs])]
        toks, pars, done = [], [], [False] * rows
        for _ in range(steps):
            par = rs.permutation(rows) if reparent else np.arange(rows)
            old = refs
            refs, tk = [], []
            for r in range(rows):
                if done[r]:
                    refs.append(old[r]); tk.append(gr.PAD)
                    continue
                g = old[par[r]].copy()
                g.carry = old[r].carry
                a = np.flatnonzero(old[par[r]].allowed())
                if reparent:
                    a = a[a != gr.EOS]
                t = int(a[rs.randint(len(a))])
                g.push(t)
                done[r] = t == gr.EOS
                refs.append(g); tk.append(t)
            toks.append(tk); pars.append(par)
            want.append(np.stack([want[-1][r] if tk[r] == gr.PAD else refs[r].allowed() for r in range(rows)]))
        assert reparent or any(done)               # the pad path is exercised
        # the device: rows with and without a carry are separate states in pass 1 (a carry tensor covers all its rows)
        groups = [list(range(rows))] if reparent else [[r for r in range(rows) if r % 2], [r for r in range(rows) if not r % 2]]
        for grp in groups:
            cb = _carry_bits([carries[r] for r in grp], dev) if carries[grp[0]] is not None else None
            st = lib.GrammarState(_grammar(), len(grp), V, dev, carry=cb, ban=ban_dev if reparent else None)
            got = torch.empty(steps + 1, len(grp), V, dtype=torch.uint8, device=dev)
            got[0] = st.mask
            tk_dev = torch.tensor(toks, dtype=torch.int64, device=dev)[:, grp].contiguous()
            pr_dev = torch.tensor(np.stack(pars), dtype=torch.int32, device=dev) if reparent else None
            for s in range(steps):
                got[s + 1] = st.advance(tk_dev[s], None if pr_dev is None else pr_dev[s])
            allowed = (got.cpu().numpy() == 0)
            np.testing.assert_array_equal(allowed, np.stack(want)[:, grp])
            act = st.active().cpu().numpy()
            for i, r in enumerate(grp):
                assert gr.bits_to_set(act[i]) == refs[r].active, r
    with pytest.raises(RuntimeError):              # a range outside the vocabulary is an error, not a launch
        lib.GrammarState(_grammar(), 2, 1200, dev)


# ---- (6) + (7) the decoder ---------------------------------------------------------------------------------------------
def _run(m, dec, ckv, B, steps, grammar=None, carry=None, sampling=None, ban=None, logprobs=False, dump=True, prefix=None):
    V = m.cfg["vocab_size"]
    n_pre = 0 if prefix is None else prefix.shape[1]
    with torch.no_grad():
        logits = torch.full((n_pre + steps, B, V), float("nan"), device=m.device) if dump else None
        out = dec.run(ckv, B, 256, steps, logits_out=logits, ban=dec.ban_mask(ban), return_logprobs=logprobs, sampling=sampling,
                      grammar=grammar, carry=carry, prefix=prefix)
        torch.cuda.synchronize()
    T = out[1] - n_pre
    ids = out[0][:B, :T + 1].cpu()
    lp = out[3][:B, :T + 1].cpu() if logprobs else None
    lg = logits[n_pre:out[1]].transpose(0, 1).cpu() if dump else None       # [B, T, V]
    return ids, lp, lg


def _host_masks(ids, carries=None, ban=None, V=1536):
    """allowed [B, T, V] for every row's history, rows frozen after their EOS; and the final GrammarRefs."""
    B, T = ids.shape[0], ids.shape[1] - 1
    out = np.zeros((B, T, V), dtype=bool)
    refs = []
    for b in range(B):
        g = gr.GrammarRef(CODEC, V=V, carry=None if carries is None else carries[b], ban=ban)
        for t in range(T):
            out[b, t] = g.allowed()
            tok = int(ids[b, t + 1])
            if tok in (gr.EOS, gr.PAD):
                out[b, t + 1:] = out[b, t]
                break
            g.push(tok)
        refs.append(g)
    return out, refs


def _live(ids):
    em = ids[:, 1:]
    e = (em == gr.EOS).long()
    return ((torch.cumsum(e, -1) - e) == 0).numpy()


def _invalid(ids, carries=None):
    return [gr.count_invalid(row[1:].tolist(), None if carries is None else carries[b], CODEC) for b, row in enumerate(ids)]


def _total_invalid(ids):
    """Invalid events over the rows of an unconstrained decode of the fixture.  These rows open with a shift past the
    segment's end, so `decode_events` drops them whole before it can call a token invalid: the invalid events are counted
    without the time limit, and with it no row may be clean."""
    per_row = _invalid(ids)
    free = [gr.count_invalid(row[1:].tolist(), None, CODEC, time_limit=False)[0] for row in ids]
    print(f"[unconstrained] (invalid, dropped) per row: {per_row}; invalid without the time limit: {free}")
    assert all(i + d > 0 for i, d in per_row)
    return sum(free)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_greedy_and_sampled_tokens_are_the_rule_under_the_host_mask(dev, dtype):
    from mrmt3.decode import Decoder, Sampling
    m = _model("t5", dtype, dev)
    d, V = m.cfg["d_model"], m.cfg["vocab_size"]
    _, enc = _enc(m, B9, seed=21)
    dec = Decoder(m, B9, STEPS, 256)
    with torch.no_grad():
        ckv = dec.cross_kv(enc.reshape(B9 * 256, d).contiguous(), B9, 256)
    rs = np.random.RandomState(3)
    carries = [gr.random_carry(rs, n=200) for _ in range(B9)]
    g = _grammar()
    for what, cr in (("no carry", None), ("carry", carries)):
        cb = None if cr is None else _carry_bits(cr, dev)
        # greedy: the argmax of the device's own logits over the host's allowed set
        ids, _, lg = _run(m, dec, ckv, B9, STEPS, grammar=g, carry=cb)
        allowed, refs = _host_masks(ids, cr)
        masked = np.where(allowed, lg.numpy(), -np.inf)
        live = _live(ids)
        want = masked.argmax(-1)
        assert (ids[:, 1:].numpy()[live] == want[live]).all(), what
        assert (ids[:, 1:].numpy()[~live] == gr.PAD).all()
        assert _invalid(ids, cr) == [(0, 0)] * B9, what
        act = dec.grammar_active(B9).cpu().numpy()
        assert [gr.bits_to_set(a) for a in act] == [r.active for r in refs], what
        # sampled, hot enough for the mask to do real work
        sp = Sampling(temperature=1.5, seed=77)
        ids, _, lg = _run(m, dec, ckv, B9, STEPS, grammar=g, carry=cb, sampling=sp)
        allowed, refs = _host_masks(ids, cr)
        T = ids.shape[1] - 1
        live = _live(ids).reshape(-1)
        masked = np.where(allowed, lg.numpy(), -np.inf).astype(np.float32).reshape(B9 * T, V)
        ref = R.sample_ref(masked, None, sp.temperature, sp.top_k, sp.top_p)
        u = R.uniform(sp.seed, np.repeat(np.arange(B9), T), np.tile(np.arange(T), B9))
        wrong, slack = ref.check(ids[:, 1:].reshape(-1).numpy(), u)
        print(f"[{what} {dtype}] sampled: {int(live.sum())} live tokens, {int(wrong[live].sum())} wrong, "
              f"{int(slack[live].sum())} by slack, allowed per step {int(allowed.sum(-1).min())}..{int(allowed.sum(-1).max())}")
        assert not wrong[live].any() and slack[live].mean() <= 0.01, what
        assert _invalid(ids, cr) == [(0, 0)] * B9, what
        act = dec.grammar_active(B9).cpu().numpy()
        assert [gr.bits_to_set(a) for a in act] == [r.active for r in refs], what
    # the same calls unconstrained: the golden weights emit near-noise, which the event decoder does not accept
    ids, _, _ = _run(m, dec, ckv, B9, STEPS, dump=False)
    assert _total_invalid(ids) > 0
    ids, _, _ = _run(m, dec, ckv, B9, STEPS, sampling=Sampling(temperature=1.5, seed=77), dump=False)
    assert _total_invalid(ids) > 0


def test_beam_search_under_a_mask_per_row(dev):
    from mrmt3.decode import Decoder
    G, k, steps = B9, 4, 48
    m = _model("t5", torch.bfloat16, dev)
    d, V = m.cfg["d_model"], m.cfg["vocab_size"]
    _, enc = _enc(m, G, seed=33)
    dec = Decoder(m, G * k, steps, 256)
    rs = np.random.RandomState(4)
    for cr in (None, [gr.random_carry(rs, n=200) for _ in range(G)]):
        cb = None if cr is None else _carry_bits([cr[r // k] for r in range(G * k)], dev)
        with torch.no_grad():
            ckv = dec.cross_kv_beam(enc.reshape(G * 256, d).contiguous(), G, k, 256)
            logits = torch.full((steps, G * k, V), float("nan"), device=dev)
            ids, done, fin = dec.run_beam(ckv, G, k, 256, steps, 0.4, None, logits_out=logits, grammar=_grammar(), carry=cb)
            torch.cuda.synchronize()
        ids, lg = ids.cpu(), logits[:done].cpu().numpy()
        bp = dec.backptr(G * k)[:done].cpu().numpy()
        ref = gr.MaskedBeamRef(G, k, V, length_penalty=0.4)
        rows = [gr.GrammarRef(CODEC, V=V, carry=None if cr is None else cr[r // k]) for r in range(G * k)]
        for t in range(done):
            allowed = np.stack([g.allowed() for g in rows])
            parents, tokens, _ = ref.step(t, lg[t], allowed)
            np.testing.assert_array_equal(bp[t, :, 0], parents, err_msg=f"parents at step {t}")
            np.testing.assert_array_equal(bp[t, :, 1], tokens, err_msg=f"tokens at step {t}")
            new = []
            for r in range(G * k):
                g = rows[parents[r]].copy()
                if tokens[r] != gr.PAD:
                    g.push(int(tokens[r]))
                new.append(g)
            rows = new
        want, best = ref.finalize(done, steps)
        np.testing.assert_array_equal(ids.numpy(), want)
        assert _invalid(ids, cr) == [(0, 0)] * G
        # the returned hypothesis' active set: its tokens pushed on the host
        act = dec.grammar_active(G).cpu().numpy()
        _, refs = _host_masks(ids, cr)
        assert [gr.bits_to_set(a) for a in act] == [r.active for r in refs]
    with torch.no_grad():
        ids, _, _ = dec.run_beam(ckv, G, k, 256, steps, 0.4, None)
    assert _total_invalid(ids.cpu()) > 0


# ---- (8) chains ------------------------------------------------------------------------------------------------------------
def _song_counts(seg_ids, eos=1):
    """A song's [n_seg, W] ids -> (est_invalid_events, est_dropped_events, notes) through the product's own pipeline."""
    import inference
    toks = inference.postprocess_batch(seg_ids, eos)
    preds = []
    for i, row in enumerate(toks):
        n = np.flatnonzero(row == vocabularies.DECODED_EOS_ID)
        row = row[:n[0]] if len(n) else row
        t0 = i * 256 / 125.0
        preds.append({"est_tokens": row, "start_time": t0 - t0 % (1 / CODEC.steps_per_second), "raw_inputs": []})
    res = metrics_utils.event_predictions_to_ns(preds, codec=CODEC, encoding_spec=note_sequences.NoteEncodingWithTiesSpec)
    return res["est_invalid_events"], res["est_dropped_events"], len(res["est_ns"].notes)


def test_songs_decode_with_no_invalid_event_end_to_end(dev):
    m = _model("segmem_v2_with_prev", torch.float32, dev)
    songs = [_enc(m, 3, seed=41)[0], _enc(m, 3, seed=42)[0]]
    plain = m.generate_songs(songs, max_length=STEPS)
    assert all(sum(_song_counts(s)[:2]) > 0 for s in plain)         # unconstrained: invalid or dropped events
    for kw in (dict(), dict(num_beams=2), dict(do_sample=True, temperature=1.5, seed=5)):
        out = m.generate_songs(songs, max_length=STEPS, constrained=True, **kw)
        counts = [_song_counts(s) for s in out]
        print(f"[songs {kw}] (invalid, dropped, notes) per song: {counts}")
        assert all(c[0] == 0 and c[1] == 0 for c in counts), kw
        assert all(s.shape == (3, STEPS) for s in out)
    # one recording through `generate` is the chain of one
    one = m.generate_beam(songs[0], max_length=STEPS, constrained=True)
    assert _song_counts(one)[:2] == (0, 0)
    assert torch.equal(one, m.generate_songs(songs[:1], max_length=STEPS, constrained=True)[0])


# ---- (9) plumbing -----------------------------------------------------------------------------------------------------------
def test_logprobs_are_normalised_over_the_allowed_set(dev):
    from mrmt3.decode import Decoder
    m = _model("t5", torch.float32, dev)
    d = m.cfg["d_model"]
    _, enc = _enc(m, B9, seed=51)
    dec = Decoder(m, B9, 48, 256)
    with torch.no_grad():
        ckv = dec.cross_kv(enc.reshape(B9 * 256, d).contiguous(), B9, 256)
    ban = [1135 + p for p in range(0, 100)]
    ids, lp, lg = _run(m, dec, ckv, B9, 48, grammar=_grammar(), logprobs=True, ban=ban)
    allowed, _ = _host_masks(ids, ban=ban)
    live = _live(ids)
    x = torch.from_numpy(np.where(allowed, lg.numpy(), -np.inf)).double()
    want = torch.log_softmax(x, -1).gather(-1, ids[:, 1:, None]).squeeze(-1).numpy()
    err = np.abs(lp[:, 1:].numpy().astype(np.float64) - want)[live].max()
    print(f"[logprobs] max|logp - fp64 over the allowed set| {err:.3e}")
    assert err <= LOGP_TOL
    assert (lp.numpy() <= 0).all() and (lp[:, 1:].numpy()[~live] == 0).all() and (lp.sum(-1).numpy() <= 0).all()
    assert not np.isin(ids.numpy(), ban).any()                      # the static ban is in the row masks
    # beam: (ids, logp) through the model call, the hypothesis' values <= 0
    bi, bl = m.generate_scored(_enc(m, 2, seed=52)[0], max_length=24, num_beams=3, constrained=True)
    assert bi.shape == bl.shape and bool((bl <= 0).all()) and _invalid(bi.cpu()) == [(0, 0)] * 2
    with pytest.raises(ValueError):
        m.generate_beam(_enc(m, 1, seed=52)[0], max_length=8, constrained=True, bad_token_ids=[1])


def test_prefix_decode_leaves_the_state_alone_until_the_tokens(dev):
    from mrmt3.decode import generate_2
    m1 = _model("segmem_v1", torch.float32, dev)
    mel, _ = _enc(m1, 3, seed=37)
    plain = generate_2(m1, mel, max_length=64)
    assert sum(_song_counts(plain)[:2]) > 0
    ids, lp = generate_2(m1, mel, max_length=64, constrained=True, return_logprobs=True)
    assert ids.shape == (3, 64) and _song_counts(ids)[:2] == (0, 0) and bool((lp <= 0).all())
    hot = generate_2(m1, mel, max_length=64, constrained=True, do_sample=True, temperature=1.5, seed=2)
    assert _song_counts(hot)[:2] == (0, 0) and not torch.equal(hot, ids)


def test_switching_the_grammar_on_and_off_on_one_decoder(dev):
    from mrmt3 import lib
    from mrmt3.decode import Decoder
    m = _model("t5", torch.bfloat16, dev)
    d = m.cfg["d_model"]
    _, enc = _enc(m, B9, seed=61)
    steps = 32

    def fresh():
        dec = Decoder(m, B9, steps, 256)
        with torch.no_grad():
            return dec, dec.cross_kv(enc.reshape(B9 * 256, d).contiguous(), B9, 256)

    lib.dispatch_counts(reset=True)
    ref_dec, ckv = fresh()
    off_ref, _, _ = _run(m, ref_dec, ckv, B9, steps, dump=False)
    off_ref2, _, _ = _run(m, ref_dec, ckv, B9, steps, dump=False)
    counts_ref, caps_ref = lib.dispatch_counts(reset=True), ref_dec.capture_count
    on_dec, ckv_on = fresh()
    on_ref, _, _ = _run(m, on_dec, ckv_on, B9, steps, grammar=_grammar(), dump=False)
    # constrained=False on a decoder of its own: ids, captures and dispatch counters of the unconstrained decode
    lib.dispatch_counts(reset=True)
    dec, ckv = fresh()
    a, _, _ = _run(m, dec, ckv, B9, steps, grammar=None, dump=False)
    a2, _, _ = _run(m, dec, ckv, B9, steps, grammar=None, dump=False)
    assert torch.equal(a, off_ref) and torch.equal(a2, off_ref2) and dec.capture_count == caps_ref == 1
    assert lib.dispatch_counts() == counts_ref
    # on -> off -> on: each switch re-captures, as a ban does; the ids are those of fresh decoders
    on1, _, _ = _run(m, dec, ckv, B9, steps, grammar=_grammar(), dump=False)
    assert dec.capture_count == 2 and torch.equal(on1, on_ref) and not torch.equal(on1, off_ref)
    on1b, _, _ = _run(m, dec, ckv, B9, steps, grammar=_grammar(max_shift_steps=100), dump=False)
    assert dec.capture_count == 2                                   # another descriptor replays the captured step
    shifts = (on1b[:, 1:] - 3)[(on1b[:, 1:] >= 3) & (on1b[:, 1:] <= 1003)]
    assert shifts.numel() == 0 or int(shifts.max()) <= 100
    off, _, _ = _run(m, dec, ckv, B9, steps, dump=False)
    assert dec.capture_count == 3 and torch.equal(off, off_ref)
    on2, _, _ = _run(m, dec, ckv, B9, steps, grammar=_grammar(), dump=False)
    assert dec.capture_count == 4 and torch.equal(on2, on_ref)
    # through the model call: the default is off
    mel, _ = _enc(m, 2, seed=62)
    assert torch.equal(m.generate_beam(mel, max_length=16), m.generate_beam(mel, max_length=16, constrained=False))
    assert torch.equal(m.generate(inputs=mel, max_length=16, constrained=True), m.generate(inputs=mel, max_length=16))


def test_inference_handler_passes_constrained_through(dev):
    import inference
    from mrmt3.synthetic import synth_audio
    audio = synth_audio(1, n_samples=3 * 16000, seed=9)[0]            # 3 s: two segments
    # a segment-memory model decodes a recording's segments one after the other: the sounding notes are handed over
    m = _model("segmem_v2_with_prev", torch.float32, dev)
    on = inference.InferenceHandler(model=m, device=dev, decode_options=True)
    toks, ft = on.inference(audio, max_length=STEPS, return_tokens=True)
    plain = on._to_event(toks, ft)

    def counts(tokens, times):
        preds = []
        for i, batch in enumerate(tokens):
            for j, row in enumerate(batch):
                n = np.flatnonzero(row == vocabularies.DECODED_EOS_ID)
                t0 = times[i][j][0]
                preds.append({"est_tokens": row[:n[0]] if len(n) else row, "start_time": t0 - t0 % 0.01, "raw_inputs": []})
        r = metrics_utils.event_predictions_to_ns(preds, codec=on.codec, encoding_spec=note_sequences.NoteEncodingWithTiesSpec)
        return r["est_invalid_events"], r["est_dropped_events"], len(r["est_ns"].notes)

    assert sum(counts(toks, ft)[:2]) > 0
    ctoks, cft = on.inference(audio, max_length=STEPS, return_tokens=True, constrained=True)
    c = counts(ctoks, cft)
    print(f"[handler] constrained (invalid, dropped, notes) = {c}; unconstrained {counts(toks, ft)}")
    assert c[0] == 0 and c[1] == 0
    # greedy on golden weights may loop on program tokens and close no note in 96 tokens; hot sampled decodes of the same
    # audio do: every seed is valid, and the seeds together return notes
    ns = on.inference(audio, max_length=STEPS, constrained=True)
    assert isinstance(ns, note_sequences.NoteSequence)
    notes = []
    for seed in range(6):
        kw = dict(max_length=STEPS, constrained=True, do_sample=True, temperature=1.5, seed=seed)
        sc = counts(*on.inference(audio, return_tokens=True, **kw))
        assert sc[:2] == (0, 0), seed
        notes.append(sc[2])
    # (`inference` itself keeps the reference's cut: a segment that never emitted EOS contributes no tokens)
    assert isinstance(on.inference(audio, **kw), note_sequences.NoteSequence)
    print(f"[handler] sampled constrained: notes per seed {notes}")
    assert sum(notes) > 0
    many = on.inference_many([audio, audio[:20000]], max_length=STEPS, return_tokens=True, constrained=True)
    assert [counts(t, f)[:2] for t, f in many] == [(0, 0), (0, 0)]
    # without decode_options the keyword is accepted and dropped, like num_beams
    off = inference.InferenceHandler(model=m, device=dev, decode_options=False)
    otoks, _ = off.inference(audio, max_length=STEPS, return_tokens=True, constrained=True)
    assert all(np.array_equal(a, b) for a, b in zip(otoks, toks))
    # the plain T5 decodes a batch's segments side by side: each row is valid given its own tie section
    t5 = _model("t5", torch.float32, dev)
    h = inference.InferenceHandler(model=t5, device=dev, decode_options=True)
    ttoks, _ = h.inference(audio, max_length=STEPS, return_tokens=True, constrained=True)
    for row in ttoks[0]:
        n = np.flatnonzero(row == vocabularies.DECODED_EOS_ID)
        assert gr.count_invalid((row[:n[0]] if len(n) else row) + 3, None, CODEC) == (0, 0)
