"""Per-token log-probabilities: the greedy tail `dec_argmax<., true>`, the beam search's per-step store and
its finalize, and teacher-forced scoring (`mrmt3_token_logprob` / `mrmt3_lmhead_logprob`, `model.score`).

Every log-probability is compared with a float64 log-softmax of f32 logits the same run produced (`logits_out`, or the
model's own forward), so only the new arithmetic is under test.  LOGP_TOL = 2e-5 absolute: an f32 tree sum of <= 1536 terms
in (0, 1] (~2e-6 relative), one log, and one subtraction of logits of magnitude < 64 (4e-6 per ulp; the tests assert the
magnitude, so the bound is honest).  Helpers are copies of tests/test_decode_gpu.py's (not imported)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from beam_ref import BeamRef  # noqa: E402

pytestmark = pytest.mark.gpu

LOGP_TOL = 2e-5
MAX_LOGIT = 64.0
NAN_ROW = 700
BAN = list(range(2, 700, 3))


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
    return m.load_golden().to(dev).eval()


def _boost_eos(w):
    w[1] *= 3.2                      # EOS competitive: rows finish at different steps


def _twin_eos(m, ids, start):
    """Make EOS the exact twin of a token the model emits: lm_head row 1 becomes a copy of the row of the first token
    above 1 that row `ids` emits for the first time at position `start` or later.  Their logits are then bit-equal and the argmax takes the lower index, so a row finishes at
    the step it would have emitted that token, deterministically and some steps into the decode; rows that never
    emit it run on.  (Scaling the EOS row until it wins, as other tests do, ends these short decodes at their first step.)"""
    seq = ids.tolist()
    cand = [t for t in dict.fromkeys(seq[1:]) if t > 1]             # emitted tokens in order of first appearance
    late = [t for t in cand if seq.index(t, 1) >= start]
    tok = int(late[0] if late else cand[-1])                        # a model that repeats itself: its newest token
    _edit(m, lambda w: w[1].copy_(w[tok]))
    return tok


def _nan_row(w):
    w[NAN_ROW] = float("nan")


def _edit(m, lm_edit):
    if lm_edit is not None:
        with torch.no_grad():
            lm_edit(m.flat.master("lm_head.weight"))
    m.engine.prepare(False)


def _enc(m, B, seed, frames=256):
    from mrmt3.synthetic import synth_mel
    mel = torch.from_numpy(synth_mel(B, frames=frames, seed=seed)).to(m.device)
    with torch.no_grad():
        return mel, m.engine.encode(mel).view(B, frames, m.cfg["d_model"])


def _ref_logp(logits, ban=None):
    """float64 log-softmax of [..., V] f32 logits, banned entries -inf first."""
    x = logits.double().clone()
    if ban:
        x[..., ban] = float("-inf")
    return torch.log_softmax(x, -1)


def _greedy(m, dec, enc, B, steps, ban=None, logprobs=True, dump=True, nan_rows=()):
    """`nan_rows`: batch rows whose cross-attention K|V are overwritten with NaN (every weight stays finite): every logit
    of those rows is NaN at every step, the other rows of the block are untouched."""
    d, V = m.cfg["d_model"], m.cfg["vocab_size"]
    with torch.no_grad():
        ckv = dec.cross_kv(enc.reshape(B * 256, d).contiguous(), B, 256)
        for r in nan_rows:
            ckv.view(ckv.shape[0], B, 256, -1)[:, r] = float("nan")
        logits = torch.full((steps, B, V), float("nan"), device=m.device) if dump else None
        out = dec.run(ckv, B, 256, steps, logits_out=logits, ban=dec.ban_mask(ban), return_logprobs=logprobs)
        assert dec.graph_captured
        torch.cuda.synchronize()
    toks, done = out[0], out[1]
    ids = toks[:B, :done + 1].cpu()
    lp = out[3][:B, :done + 1].cpu() if logprobs else None
    lg = logits[:done].transpose(0, 1).cpu() if dump else None       # [B, done, V]
    return ids, lp, lg


def _live_mask(ids, eos):
    """[B, T] True up to and including each row's first EOS."""
    emitted = ids[:, 1:]
    after = torch.cumsum((emitted == eos).long(), -1) - (emitted == eos).long()
    return after == 0


GREEDY = [(dt, B, ban) for dt in (torch.float32, torch.bfloat16) for B in (3, 9) for ban in (None, BAN)]


@pytest.mark.parametrize("dtype,B,ban", GREEDY,
                         ids=[f"{'fp32' if dt == torch.float32 else 'bf16'}-b{B}-{'ban' if ban else 'plain'}" for dt, B, ban in GREEDY])
def test_greedy_logprobs_match_fp64_log_softmax_of_the_dumped_logits(dev, dtype, B, ban):
    from mrmt3.decode import Decoder
    m = _model("t5", dtype, dev)
    _edit(m, None)
    _, enc = _enc(m, B, seed=13 + B)
    dec = Decoder(m, B, 32, 256)
    first, _, _ = _greedy(m, dec, enc, B, 32, ban=ban, logprobs=False, dump=False)
    _twin_eos(m, first[0], 8)                                       # row 0 finishes at step 7 or later
    ids, lp, lg = _greedy(m, dec, enc, B, 32, ban=ban)
    assert lp.dtype == torch.float32 and lp.shape == ids.shape
    assert float(lg.abs().max()) < MAX_LOGIT
    ref = _ref_logp(lg, ban).gather(-1, ids[:, 1:, None]).squeeze(-1)
    live = _live_mask(ids, m.cfg["eos_token_id"])
    err = float((lp[:, 1:].double() - ref)[live].abs().max())
    print(f"[greedy {dtype} B={B} ban={bool(ban)}] max|logp - fp64| {err:.3e} over {int(live.sum())} tokens, "
          f"{int((~live).sum())} pad positions, min logp {float(ref[live].min()):.3f}")
    assert err <= LOGP_TOL, err
    assert (lp[:, 0] == 0).all()                                    # the start token
    assert (lp[:, 1:][~live] == 0).all()                            # pads of rows that had finished: exactly 0.0
    assert (ids[:, 1:][~live] == m.cfg["pad_token_id"]).all()
    assert (~live).any() and int(live.sum()) > B, "the fixture must finish a row, and not every row at once"
    if ban:
        assert not np.isin(ids[:, 1:].numpy(), ban).any()
    plain, _, _ = _greedy(m, dec, enc, B, 32, ban=ban, logprobs=False, dump=False)
    assert torch.equal(plain, ids)                                  # same ids without the feature


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_greedy_logprob_of_a_nan_logit_is_nan(dev, dtype):
    """lm_head row NAN_ROW is NaN (planted as tests/test_decode_gpu.py does; every other weight finite): that logit is NaN
    in every row and step, the argmax takes it, and its log-probability is NaN; with the token banned the NaN is gone."""
    from mrmt3.decode import Decoder
    m = _model("t5", dtype, dev)
    _edit(m, _nan_row)
    _, enc = _enc(m, 3, seed=5)
    dec = Decoder(m, 3, 16, 256)
    ids, lp, lg = _greedy(m, dec, enc, 3, 16)
    assert torch.isnan(lg[..., NAN_ROW]).all()
    assert ids.shape == (3, 17) and (ids[:, 1:] == NAN_ROW).all()   # ran to the end, in range
    assert torch.isnan(lp[:, 1:]).all() and (lp[:, 0] == 0).all()
    plain, _, _ = _greedy(m, dec, enc, 3, 16, logprobs=False, dump=False)
    assert torch.equal(plain, ids)
    ids, lp, lg = _greedy(m, dec, enc, 3, 16, ban=[NAN_ROW])
    assert (ids >= 0).all() and (ids < m.cfg["vocab_size"]).all() and not (ids == NAN_ROW).any()
    ref = _ref_logp(lg, [NAN_ROW]).gather(-1, ids[:, 1:, None]).squeeze(-1)
    live = _live_mask(ids, m.cfg["eos_token_id"])
    assert float((lp[:, 1:].double() - ref)[live].abs().max()) <= LOGP_TOL


@pytest.mark.parametrize("dtype,B", [(torch.float32, 3), (torch.bfloat16, 9)], ids=["fp32-b3", "bf16-b9"])
def test_a_nan_row_beside_finite_rows(dev, dtype, B):
    """One batch row's logits are NaN (planted through its cross-attention K|V; the weights are finite) inside a block of
    8 rows whose other rows are finite: that row returns NaN at every step and emits token 0 (torch.argmax's first NaN),
    its neighbours keep their fp64 accuracy, and the decode runs to its end with every id in range."""
    from mrmt3.decode import Decoder
    m = _model("t5", dtype, dev)
    _edit(m, None)
    _, enc = _enc(m, B, seed=21 + B)
    dec = Decoder(m, B, 16, 256)
    bad = 1
    ids, lp, lg = _greedy(m, dec, enc, B, 16, nan_rows=(bad,))
    good = [b for b in range(B) if b != bad]
    assert torch.isnan(lg[bad]).all() and not torch.isnan(lg[good]).any()
    assert (ids >= 0).all() and (ids < m.cfg["vocab_size"]).all() and ids.shape[1] == 17
    assert (ids[bad, 1:] == 0).all() and torch.isnan(lp[bad, 1:]).all() and lp[bad, 0] == 0
    assert float(lg[good].abs().max()) < MAX_LOGIT
    ref = _ref_logp(lg[good]).gather(-1, ids[good, 1:, None]).squeeze(-1)
    live = _live_mask(ids[good], m.cfg["eos_token_id"])
    assert float((lp[good, 1:].double() - ref)[live].abs().max()) <= LOGP_TOL
    plain, _, _ = _greedy(m, dec, enc, B, 16, logprobs=False, dump=False, nan_rows=(bad,))
    assert torch.equal(plain, ids)


def test_prefix_steps_write_nothing_and_generate_2_returns_logprobs(dev):
    """The memory-prefixed decode (`generate_2`): the 64 prefix steps write no log-probability, token step t writes column
    t + 1 (not prefix + t + 1), and what was there beyond the last step stays."""
    from mrmt3.decode import Decoder, generate_2
    from mrmt3.synthetic import synth_labels
    B, n_pre, steps = 2, 64, 16
    m = _model("segmem_v1", torch.float32, dev)
    _edit(m, _boost_eos)
    eng, d, V = m.engine, m.cfg["d_model"], m.cfg["vocab_size"]
    mel, enc = _enc(m, B, seed=37)
    with torch.no_grad():
        pre_ids = torch.from_numpy(synth_labels(B, 256, seed=38)).clamp(min=0).to(dev)
        pre = eng.segmem(pre_ids, B, 256)[:, :n_pre].float().contiguous()
        dec = Decoder(m, B, n_pre + steps, 256)
        dec.logp_buffer().fill_(7.0)                                # sentinel: no step may touch what it does not own
        ckv = dec.cross_kv(enc.reshape(B * 256, d).contiguous(), B, 256)
        logits = torch.full((n_pre + steps, B, V), float("nan"), device=dev)
        toks, done, fin, lp = dec.run(ckv, B, 256, steps, prefix=pre, logits_out=logits, return_logprobs=True)
        torch.cuda.synchronize()
    T = done - n_pre
    ids, lp_all = toks[:B, :T + 1].cpu(), lp[:B].cpu()
    lg = logits[n_pre:done].transpose(0, 1).cpu()
    assert float(lg.abs().max()) < MAX_LOGIT
    ref = _ref_logp(lg).gather(-1, ids[:, 1:, None]).squeeze(-1)
    live = _live_mask(ids, m.cfg["eos_token_id"])
    assert float((lp_all[:, 1:T + 1].double() - ref)[live].abs().max()) <= LOGP_TOL
    assert (lp_all[:, 0] == 0).all() and (lp_all[:, 1:T + 1][~live] == 0).all()
    assert (lp_all[:, T + 1:] == 7.0).all()                         # 64 prefix steps + T token steps wrote T columns
    a, alp = generate_2(m, mel, max_length=64, return_logprobs=True)
    assert torch.equal(a, generate_2(m, mel, max_length=64))
    assert alp.shape == a.shape and alp.dtype == torch.float32 and (alp[:, 0] == 0).all()
    assert bool((alp <= 0).all())
    assert bool((alp[:, 1:][a[:, 1:] != 0] < 0).any())


def test_logprobs_across_decode_batches_of_256(dev):
    """More rows than one decode batch holds: `generate` (257 rows) and `generate_beam` (k = 2, 129 groups) decode in two
    batches and stack ids and log-probabilities alike; each part equals that part decoded on its own.  This checks the
    stacking, not the arithmetic: a part encoded on its own runs the f32 encoder GEMMs at another row count (other tiles,
    another order of additions, ~1e-6 in the logits), so the ids must agree and the values to 1e-4."""
    from mrmt3.decode import generate, generate_beam
    m = _model("t5", torch.float32, dev)
    _edit(m, _boost_eos)
    mel, _ = _enc(m, 257, seed=53)

    def check(fn, x, cut):
        ids, lp = fn(x)
        assert lp.shape == ids.shape and lp.dtype == torch.float32
        at = 0
        for part in (x[:cut], x[cut:]):
            pi, pl = fn(part)
            n, w = pi.shape
            assert torch.equal(ids[at:at + n, :w], pi) and float((lp[at:at + n, :w] - pl).abs().max()) <= 1e-4
            assert (ids[at:at + n, w:] == 0).all() and (lp[at:at + n, w:] == 0).all()
            at += n
        assert at == x.shape[0]

    check(lambda x: generate(m, x, max_length=8, return_logprobs=True), mel, 256)
    check(lambda x: generate_beam(m, x, num_beams=2, max_length=6, length_penalty=0.4, return_logprobs=True), mel[:129], 128)


def test_inference_with_confidence_end_to_end(dev):
    """audio -> notes with a confidence each: the same notes as without, `min_confidence` keeps exactly the notes at or
    above it, `return_tokens` hands the log-probabilities out under the tokens' cuts; `inference_many` agrees."""
    import inference
    from mrmt3.synthetic import synth_audio
    m = _model("t5", torch.float32, dev)
    _edit(m, None)
    h = inference.InferenceHandler(model=m, device=dev)
    audio = synth_audio(1, n_samples=3 * 32768, seed=9)[0]
    first, _ = h.inference(audio, max_length=48, return_tokens=True)
    _twin_eos(m, torch.from_numpy(first[0][0] + 3), 20)             # un-post-processed ids of segment 0
    plain = h.inference(audio, max_length=48)
    scored = h.inference(audio, max_length=48, with_confidence=True)
    toks, ft, lps = h.inference(audio, max_length=48, with_confidence=True, return_tokens=True)
    toks0, _ = h.inference(audio, max_length=48, return_tokens=True)
    assert len(toks) == len(lps) == len(toks0)
    for t, t0, l in zip(toks, toks0, lps):
        assert np.array_equal(t, t0) and l.shape == t.shape and l.dtype == np.float32
        assert (l <= 0).all() and (l[t != -1] < 0).any()
    assert scored.notes == plain.notes
    assert all(0.0 < n.confidence <= 1.0 for n in scored.notes) and all(n.confidence == 1.0 for n in plain.notes)
    print(f"[inference] {len(scored.notes)} notes, confidences {sorted(round(n.confidence, 4) for n in scored.notes)[:8]} ...")
    if scored.notes:
        floor = sorted(n.confidence for n in scored.notes)[len(scored.notes) // 2]
        kept = h.inference(audio, max_length=48, min_confidence=floor)
        want = [n for n in scored.notes if n.confidence >= floor]
        assert [(n.start_time, n.pitch, n.program, n.is_drum) for n in kept.notes] == \
            [(n.start_time, n.pitch, n.program, n.is_drum) for n in want]
    many = h.inference_many([audio, audio[:32768]], max_length=48, with_confidence=True)
    assert many[0].notes == scored.notes
    assert np.allclose([n.confidence for n in many[0].notes], [n.confidence for n in scored.notes], atol=1e-4)


def test_logprobs_are_part_of_the_capture_key(dev):
    """greedy, greedy with log-probabilities, greedy again on one handle: the first and third are bit-equal, every run
    replays a captured graph, and the plain run launches what it launches on a handle that never enabled the feature."""
    from mrmt3 import lib
    from mrmt3.decode import Decoder
    m = _model("t5", torch.bfloat16, dev)
    _edit(m, _boost_eos)
    _, enc = _enc(m, 4, seed=31)

    def plain(dec):
        lib.dispatch_counts(reset=True)
        ids, _, _ = _greedy(m, dec, enc, 4, 24, logprobs=False, dump=False)
        return ids, lib.dispatch_counts()

    fresh = Decoder(m, 4, 24, 256)
    f1, _ = plain(fresh)
    f3, fresh_counts = plain(fresh)
    dec = Decoder(m, 4, 24, 256)
    g1, _ = plain(dec)
    g2, lp, _ = _greedy(m, dec, enc, 4, 24, dump=False)
    g3, counts = plain(dec)
    assert torch.equal(g1, g3) and torch.equal(g1, g2) and torch.equal(g1, f1) and torch.equal(f1, f3)
    assert counts == fresh_counts, (counts, fresh_counts)
    assert torch.isfinite(lp).all() and (lp[:, 1:] <= 0).all()


@pytest.mark.parametrize("dtype,k", [(torch.float32, 2), (torch.bfloat16, 4)], ids=["fp32-k2", "bf16-k4"])
def test_beam_logprobs_follow_the_best_hypothesis(dev, dtype, k):
    from mrmt3.decode import Decoder, generate_beam
    G, steps, lpen = 2, 24, 0.4
    m = _model("t5", dtype, dev)
    _edit(m, _boost_eos)
    cfg, d, V = m.cfg, m.cfg["d_model"], m.cfg["vocab_size"]
    mel, enc = _enc(m, G, seed=29)
    dec = Decoder(m, G * k, steps, 256)
    with torch.no_grad():
        ckv = dec.cross_kv_beam(enc.reshape(G * 256, d).contiguous(), G, k, 256)
        logits = torch.full((steps, G * k, V), float("nan"), device=dev)
        ids, done, fin, lp = dec.run_beam(ckv, G, k, 256, steps, lpen, dec.ban_mask(BAN), logits_out=logits,
                                          return_logprobs=True)
        torch.cuda.synchronize()
        ids, lp, logits = ids.cpu(), lp.cpu(), logits[:done].cpu()
        plain = generate_beam(m, mel, num_beams=k, max_length=steps, length_penalty=lpen, bad_token_ids=BAN).cpu()
        ids2, lp2 = m.generate_scored(mel, max_length=steps, num_beams=k, length_penalty=lpen, bad_token_ids=BAN)
    assert torch.equal(ids, plain) and torch.equal(ids2.cpu(), plain) and torch.equal(lp2.cpu(), lp)
    assert lp.shape == ids.shape and lp.dtype == torch.float32
    assert float(logits.abs().max()) < MAX_LOGIT
    # the float64 search on the copied logits
    ref = BeamRef(G, k, V, eos=cfg["eos_token_id"], pad=cfg["pad_token_id"], start=cfg["decoder_start_token_id"],
                  length_penalty=lpen, ban=BAN)
    logp, T = [], 0
    for t in range(done):
        if ref.all_done:
            break
        ref.step(t, logits[t].double().numpy())
        logp.append(_ref_logp(logits[t]).numpy())                   # the reference's per-step log_softmax (the search bans after it)
        T = t + 1
    out, best = ref.finalize(T, steps)
    assert (ids.numpy() == out).all()
    for g in range(G):
        score, end, row = best[g]
        want = np.zeros(ids.shape[1])
        by_eos = end < T
        if by_eos and 1 + end < ids.shape[1]:
            want[1 + end] = logp[end][row, cfg["eos_token_id"]]
        r = row
        for s in range(end - 1, -1, -1):
            p, tk = ref.bp[s]
            want[1 + s] = logp[s][p[r], tk[r]]
            r = int(p[r])
        n_tok = end + (1 if by_eos else 0)
        raw = score * (end + 1) ** lpen                             # the scorer divides by cur_len ** length_penalty
        got = lp[g].double().numpy()
        err = np.abs(got - want).max()
        print(f"[beam k={k} g={g}] {n_tok} tokens ({'EOS' if by_eos else 'running beam'}), max|logp - fp64| {err:.3e}, "
              f"sum {got.sum():.6f} vs raw score {raw:.6f}")
        assert err <= LOGP_TOL, err
        assert abs(got.sum() - raw) <= LOGP_TOL * n_tok, (got.sum(), raw)
        assert (got[1 + n_tok:] == 0).all() and got[0] == 0


def _score_inputs(variant, dev, B=3, L=32):
    from mrmt3.synthetic import synth_labels, synth_mel
    mel = torch.from_numpy(synth_mel(B, seed=17)).to(dev)
    labels = torch.from_numpy(synth_labels(B, L, seed=19, full=False, mean_len=12)).to(dev)
    prev = None
    if variant != "t5":
        prev = torch.from_numpy(synth_labels(B, L, seed=23, full=False, mean_len=12)).to(dev)
    return mel, labels, prev


SCORE = [(v, dt) for v in ("t5", "segmem_v2_with_prev") for dt in (torch.float32, torch.bfloat16)]


@pytest.mark.parametrize("variant,dtype", SCORE, ids=[f"{v}-{'fp32' if dt == torch.float32 else 'bf16'}" for v, dt in SCORE])
def test_score_matches_the_forward_logits_and_eval_loss(dev, variant, dtype):
    from mrmt3.trainer import Trainer
    m = _model(variant, dtype, dev)
    mel, labels, prev = _score_inputs(variant, dev)
    cp = lambda t: None if t is None else t.clone()
    assert (labels == -100).any() and (labels[:, 0] != -100).all()
    with torch.no_grad():
        sc = m.score(mel, labels, cp(prev))
        logits = m(inputs=mel, labels=labels, targets_prev=cp(prev)).cpu()
        small = m.score(mel, labels, cp(prev), chunk_rows=40)       # 96 rows in chunks of 40, 40, 16
        loss = float(Trainer(m).eval_loss(mel, labels, cp(prev)))
    assert sc.shape == labels.shape and sc.dtype == torch.float32
    assert torch.equal(small, sc)
    assert float(logits.abs().max()) < MAX_LOGIT
    lab, sc = labels.cpu(), sc.cpu()
    keep = lab != -100
    ref = _ref_logp(logits).gather(-1, lab.clamp(min=0)[..., None]).squeeze(-1)
    err = float((sc.double() - ref)[keep].abs().max())
    assert err <= LOGP_TOL, err
    assert (sc[~keep] == 0).all()
    # eval_loss reads the same f32 logits (the same mrmt3_gemm_nt product), so the two are held against each other, not
    # each against an exact value: 1e-6 relative per token for the f32 steps both take (subtractions, log, the 1 / count
    # scale and the cast of the loss), plus the reduction-order difference: the CE kernel and the scorer add the same
    # <= 1536 exponentials in two different f32 orders, each within ~2e-6 relative of the exact sum, so their logs differ by
    # at most 4e-6.  Measured on an MI355X: see profiles/r09_decode_logprobs.txt.
    mine = float(-sc.double().sum() / keep.sum())
    bound = 1e-6 * abs(loss) + 4e-6
    print(f"[score {variant} {dtype}] max|score - fp64| {err:.3e}; -sum/count {mine:.7f} vs eval_loss {loss:.7f}: "
          f"difference {abs(mine - loss):.3e} (bound {bound:.3e})")
    assert abs(mine - loss) <= bound, (mine, loss)


def test_decoder_logprobs_equal_the_teacher_forced_score_of_its_own_tokens(dev):
    """The cross-check: the fp32 decoder's log-probabilities for the tokens it chose against `model.score` of those
    tokens through the training forward.  The two paths compute the logits with different kernels; the bound is twice
    the largest logit difference between them at the scored positions (measured here) plus LOGP_TOL."""
    from mrmt3.decode import Decoder
    B, steps = 3, 24
    m = _model("t5", torch.float32, dev)
    _edit(m, None)
    mel, enc = _enc(m, B, seed=43)
    dec = Decoder(m, B, steps, 256)
    first, _, _ = _greedy(m, dec, enc, B, steps, logprobs=False, dump=False)
    _twin_eos(m, first[0], 8)
    ids, lp, lg = _greedy(m, dec, enc, B, steps)
    live = _live_mask(ids, m.cfg["eos_token_id"])
    labels = torch.where(live, ids[:, 1:], torch.full_like(ids[:, 1:], -100)).to(dev).contiguous()
    with torch.no_grad():
        sc = m.score(mel, labels).cpu()
        fwd = m(inputs=mel, labels=labels).cpu()
    gap = float((fwd.double() - lg.double()).abs().max(-1).values[live].max())
    diff = float((sc.double() - lp[:, 1:].double())[live].abs().max())
    print(f"[decode vs score] max|forward logits - decode logits| {gap:.3e}; max|score - decoder logp| {diff:.3e} "
          f"over {int(live.sum())} tokens")
    assert int(live.sum()) > B and (~live).any()
    assert diff <= 2 * gap + LOGP_TOL, (diff, gap)
    assert (sc[~live] == 0).all() and (lp[:, 1:][~live] == 0).all()


def test_songs_logprobs_equal_each_recording_alone(dev):
    from mrmt3.decode import generate, generate_songs
    from mrmt3.synthetic import synth_mel
    m = _model("segmem_v2_with_prev", torch.float32, dev)
    _edit(m, _boost_eos)
    songs = [torch.from_numpy(synth_mel(n, frames=256, seed=40 + n)).to(dev) for n in (2, 1, 2)]
    ML = 32
    ids, lps = generate_songs(m, songs, max_length=ML, return_logprobs=True)
    plain = generate_songs(m, songs, max_length=ML)
    for s, song in enumerate(songs):
        a, alp = generate(m, song, max_length=ML, return_logprobs=True)
        assert ids[s].shape == lps[s].shape == (song.shape[0], ML) and lps[s].dtype == torch.float32
        assert torch.equal(ids[s], a) and torch.equal(ids[s], plain[s]), s
        assert torch.equal(lps[s], alp), s                          # bit for bit
        assert (lps[s][:, 0] == 0).all() and bool((lps[s] < 0).any())
    # one beam group per recording: the segment-memory branch of generate_beam, and the beam rows cut / padded to ML
    from mrmt3.decode import generate_beam
    bids, blps = generate_songs(m, songs, max_length=ML, num_beams=2, length_penalty=0.4, return_logprobs=True)
    for s, song in enumerate(songs):
        a, alp = generate_beam(m, song, num_beams=2, max_length=ML, length_penalty=0.4, return_logprobs=True)
        assert bids[s].shape == blps[s].shape == (song.shape[0], ML) and blps[s].dtype == torch.float32
        assert torch.equal(bids[s], a) and torch.equal(blps[s], alp), s
        assert (blps[s] <= 0).all() and (blps[s][:, 0] == 0).all() and bool((blps[s] < 0).any())
