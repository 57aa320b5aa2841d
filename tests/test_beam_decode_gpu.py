"""Beam search and banned tokens on the MI355X decoder (csrc/decode_tail.hip dec_beam_select / dec_beam_reorder /
dec_beam_finalize_kernel, dec_argmax<true>), scored against the float64 host restatement of HF 4.18's beam search
(tests/beam_ref.py) and the float64 teacher-forced decoder (oracle.t5_ref.decode_step_logits).

  (a) selection exact: every step's copied logits, rerun through the host scorer, give the same parents, tokens,
      hypotheses and final ids; beam scores agree to fp32 accumulation accuracy, and the fixture's smallest rank / done
      margins are asserted to exceed that tolerance so the comparison means something;
  (b) cache right: each final row's history, teacher-forced through the fp64 decoder, reproduces the logits copied
      from whichever row held each prefix at each step (a wrong KV-cache reorder breaks this);
  (c) bans; (d) lockstep songs; (e) graph reuse, mode switches, a full-length run, a NaN logit; (f) end to end against
      an fp64 CPU beam search.
Helpers are copies of tests/test_decode_gpu.py's (not imported)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from beam_ref import BeamRef, beam_search  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_MAX_ABS = 1e-5          # as tests/test_decode_gpu.py (b)
BF16_MAX_ABS = 0.1           # as tests/test_decode_gpu.py (c)
BF16_ROW_REL = 1.2e-2
BF16 = lambda t: t.float().bfloat16().double()


def _tol(s):
    """fp32 beam-score accuracy: log-softmax rounding plus one rounding per accumulated step."""
    return 1e-5 + 4e-6 * np.abs(s)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(variant, dtype, dev):
    from mrmt3.synthetic import T5_SMALL
    if variant == "t5":
        from models.t5 import T5ForConditionalGeneration
        m = T5ForConditionalGeneration(T5_SMALL, compute_dtype=dtype)
    else:
        from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev
        m = T5SegMemV2WithPrev(T5_SMALL, segmem_num_layers=1, segmem_length=64, compute_dtype=dtype)
    return m.load_golden().to(dev).eval()


def _dec_keys(cfg):
    ks = ["decoder_embed_tokens.weight", "lm_head.weight", "decoder.final_layer_norm.weight"]
    for i in range(cfg["num_decoder_layers"]):
        b = f"decoder.block.{i}.layer"
        ks += [f"{b}.0.layer_norm.weight", f"{b}.1.layer_norm.weight", f"{b}.2.layer_norm.weight"]
        ks += [f"{b}.0.SelfAttention.{n}.weight" for n in "qkvo"]
        ks += [f"{b}.1.EncDecAttention.{n}.weight" for n in "qo"]
        ks += [f"{b}.2.DenseReluDense.{n}.weight" for n in ("wi_0", "wi_1", "wo")]
    return ks


def _master_sd(m):
    return {k: m.flat.master(k).detach().double().cpu() for k in _dec_keys(m.cfg)}


def _engine_sd(m):
    eng, cfg = m.engine, m.cfg
    inner, dff = eng.inner, cfg["d_ff"]
    sd = _master_sd(m)
    W = lambda n: eng.W(n).detach().double().cpu()
    sd["lm_head.weight"] = W("lm_head")
    for i in range(cfg["num_decoder_layers"]):
        b = f"decoder.block.{i}.layer"
        qkv, wi = W(f"decoder.{i}.qkv"), W(f"decoder.{i}.wi")
        for j, n in enumerate("qkv"):
            sd[f"{b}.0.SelfAttention.{n}.weight"] = qkv[j * inner:(j + 1) * inner]
        sd[f"{b}.0.SelfAttention.o.weight"] = W(f"decoder.{i}.o")
        sd[f"{b}.1.EncDecAttention.q.weight"] = W(f"decoder.{i}.cq")
        sd[f"{b}.1.EncDecAttention.o.weight"] = W(f"decoder.{i}.co")
        sd[f"{b}.2.DenseReluDense.wi_0.weight"], sd[f"{b}.2.DenseReluDense.wi_1.weight"] = wi[:dff], wi[dff:]
        sd[f"{b}.2.DenseReluDense.wo.weight"] = W(f"decoder.{i}.wo")
    return sd


def _boost_eos(w):
    w[1] *= 3.2                      # EOS competitive: hypotheses at different steps


def _no_eos(w):
    w[1].zero_()                     # EOS never wins: every step runs


NAN_ROW = 700


def _nan_row(w):
    w[NAN_ROW] = float("nan")


def _edit(m, lm_edit):
    if lm_edit is not None:
        with torch.no_grad():
            lm_edit(m.flat.master("lm_head.weight"))
    m.engine.prepare(False)


def _enc(m, G, seed, frames=256):
    from mrmt3.synthetic import synth_mel
    mel = torch.from_numpy(synth_mel(G, frames=frames, seed=seed)).to(m.device)
    with torch.no_grad():
        return mel, m.engine.encode(mel).view(G, frames, m.cfg["d_model"])


def _beam(m, G, k, steps, seed=7, lp=1.0, ban=None, dec=None):
    """Beam decode of G synthetic segments with logits_out; everything on the host afterwards."""
    from mrmt3.decode import Decoder
    cfg, d, Lc = m.cfg, m.cfg["d_model"], 256
    _, enc = _enc(m, G, seed)
    dec = dec or Decoder(m, G * k, steps, Lc)
    with torch.no_grad():
        ckv = dec.cross_kv_beam(enc.reshape(G * Lc, d).contiguous(), G, k, Lc)
        logits = torch.full((steps, G * k, cfg["vocab_size"]), float("nan"), device=m.device)
        ids, done, fin = dec.run_beam(ckv, G, k, Lc, steps, lp, dec.ban_mask(ban), logits_out=logits)
        torch.cuda.synchronize()
    L, inner = cfg["num_decoder_layers"], m.engine.inner
    kv = ckv.view(L, G * k, Lc, 2 * inner).cpu()
    hy = dec.hyps(G).cpu()
    return SimpleNamespace(G=G, k=k, steps=steps, lp=lp, ban=ban, ids=ids.cpu(), done=done, fin=fin, dec=dec,
                           logits=logits[:done].cpu(), bp=dec.backptr(G * k)[:done].cpu(),
                           scores=dec.beam_scores(G * k).cpu(), hyps=hy, hyp_f=hy.view(torch.float32),
                           ck=kv[..., :inner], cv=kv[..., inner:])


def _check_selection(m, r, check_margins=True):
    """(a): rerun the float64 scorer on the copied logits, step by step."""
    cfg = m.cfg
    ref = BeamRef(r.G, r.k, cfg["vocab_size"], eos=cfg["eos_token_id"], pad=cfg["pad_token_id"],
                  start=cfg["decoder_start_token_id"], length_penalty=r.lp, ban=r.ban)
    T = 0
    for t in range(r.done):
        if ref.all_done:                     # steps the poll loop ran past the end: every group pads in place
            assert (r.bp[t, :, 0] == torch.arange(r.G * r.k)).all() and (r.bp[t, :, 1] == cfg["pad_token_id"]).all()
            continue
        p, tk, sc = ref.step(t, r.logits[t].double().numpy())
        T = t + 1
        bad = np.nonzero((r.bp[t, :, 0].numpy() != p) | (r.bp[t, :, 1].numpy() != tk))[0]
        assert len(bad) == 0, f"step {t}: rows {bad.tolist()} parents {r.bp[t, bad, 0].tolist()} vs {p[bad].tolist()}, " \
                              f"tokens {r.bp[t, bad, 1].tolist()} vs {tk[bad].tolist()}"
    assert r.fin == (T - 1 if ref.all_done else -1), (r.fin, T, ref.all_done)
    live = np.repeat(~np.asarray(ref.done), r.k)
    d = np.abs(r.scores.double().numpy() - ref.scores)[live]
    assert (d <= _tol(ref.scores[live])).all(), d.max()
    err = [float(d.max()) if len(d) else 0.0]
    out, best = ref.finalize(T, r.steps)
    for g in range(r.G):                        # the hypothesis records after finalize, in list order
        n = int(r.hyps[g, 0])
        got = [(float(r.hyp_f[g, 4 + 3 * i]), int(r.hyps[g, 5 + 3 * i]), int(r.hyps[g, 6 + 3 * i])) for i in range(n)]
        want = ref.hyps[g]
        assert [e[1:] for e in got] == [e[1:] for e in want], (g, got, want)
        assert all(abs(a[0] - b[0]) <= _tol(b[0]) for a, b in zip(got, want)), (g, got, want)
        err += [abs(a[0] - b[0]) for a, b in zip(got, want)]
        assert int(r.hyps[g, 3]) == len(ref.history(best[g][1], best[g][2]))
    assert r.ids.shape == out.shape and (r.ids.numpy() == out).all(), (r.ids, out)
    if check_margins:
        # a pass means something only if no decision was closer than the GPU's score error (the largest is the
        # accumulated beam score of the last step): every rank and done-test gap must clear 2x that, and 1e-5
        rank_gap = min(ref.margins)
        done_gap = min(ref.done_margins) if ref.done_margins else float("inf")
        need = max(1e-5, 2 * max(err))
        print(f"[a G={r.G} k={r.k}] {T} steps, smallest rank gap {rank_gap:.3e}, done/admission gap {done_gap:.3e}, "
              f"score error {max(err):.3e}, hypotheses {[len(h) for h in ref.hyps]}")
        assert rank_gap > need and done_gap > need, (rank_gap, done_gap, need)
    return ref, T


def _check_cache(m, r, ref, T):
    """(b): the fp64 teacher-forced logits along every final row's history = the copied logits of the row that held
    each prefix at each step."""
    from oracle import t5_ref
    rows = r.G * r.k
    ids = torch.zeros(rows, T, dtype=torch.long)
    holder = np.zeros((rows, T), dtype=np.int64)
    for row in range(rows):
        ids[row] = torch.tensor(ref.history(T, row)[:T])
        cur = row
        for s in range(T - 1, -1, -1):
            cur = int(ref.bp[s][0][cur])
            holder[row, s] = cur
    got = torch.stack([r.logits[s, holder[:, s]] for s in range(T)], 1)          # [rows, T, V]
    sd, rnd = (_master_sd(m), None) if m.engine.dt == torch.float32 else (_engine_sd(m), BF16)
    with torch.no_grad():
        exp = t5_ref.decode_step_logits(sd, m.cfg, ids, r.ck, r.cv, rnd=rnd)
    d = (got.double() - exp).abs()
    mx = float(d.max())
    rel = float(((got.double() - exp).norm(dim=-1) / exp.norm(dim=-1)).max())
    moved = int((holder != np.arange(rows)[:, None]).sum())
    print(f"[b G={r.G} k={r.k}] {T} steps, {moved} (row, step) prefixes held by another row: max|d| {mx:.3e} rel {rel:.3e}")
    assert moved > 0
    if m.engine.dt == torch.float32:
        assert mx <= FP32_MAX_ABS, mx
    else:
        assert mx <= BF16_MAX_ABS and rel <= BF16_ROW_REL, (mx, rel)


CASES = [
    # id, dtype, k, G, steps, lm_edit, length penalty, ban, seed      (bf16 with > 8 rows = the MFMA step)
    ("fp32-k2-g1", torch.float32, 2, 1, 48, None, 1.0, None, 19),
    ("fp32-k4-g3-eos", torch.float32, 4, 3, 48, _boost_eos, 0.4, None, 29),
    ("bf16-k8-g1", torch.bfloat16, 8, 1, 32, None, 0.4, None, 25),
    ("bf16-k3-g3-ban", torch.bfloat16, 3, 3, 40, None, 1.0, list(range(2, 700, 3)), 41),
    ("bf16-k8-g2-eos", torch.bfloat16, 8, 2, 48, _boost_eos, 0.4, None, 33),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_beam_selection_and_cache_match_fp64(dev, case):
    tag, dtype, k, G, steps, lm_edit, lp, ban, seed = case
    m = _model("t5", dtype, dev)
    _edit(m, lm_edit)
    r = _beam(m, G, k, steps, seed=seed, lp=lp, ban=ban)
    assert r.dec.graph_captured
    ref, T = _check_selection(m, r)
    if lm_edit is _boost_eos:
        assert sum(len(h) for h in ref.hyps) > 0 and any(e[1] < T for h in ref.hyps for e in h), "no EOS hypothesis"
    if ban:
        assert not np.isin(r.bp[:, :, 1].numpy(), ban).any()
    _check_cache(m, r, ref, T)


@pytest.mark.parametrize("dtype,B", [(torch.float32, 2), (torch.bfloat16, 16)], ids=["fp32-gemv", "bf16-mfma"])
def test_masked_greedy_is_the_argmax_of_the_unbanned_logits(dev, dtype, B):
    """(c) greedy: banned ids (the NaN logit among them) score -inf before the argmax; ties and NaN rules otherwise as
    torch.argmax.  A second decode without the ban on the same handle is the plain greedy decode again."""
    from mrmt3.decode import Decoder
    m = _model("t5", dtype, dev)
    _edit(m, _nan_row)
    cfg, d = m.cfg, m.cfg["d_model"]
    _, enc = _enc(m, B, seed=5)
    ban = [NAN_ROW] + list(range(3, 1536, 2))
    dec = Decoder(m, B, 24, 256)
    with torch.no_grad():
        ckv = dec.cross_kv(enc.reshape(B * 256, d).contiguous(), B, 256)
        logits = torch.full((24, B, cfg["vocab_size"]), float("nan"), device=dev)
        toks, done, fin = dec.run(ckv, B, 256, 24, logits_out=logits, ban=dec.ban_mask(ban))
        toks = toks[:B, :done + 1].cpu()
        assert dec.graph_captured
        plain, done2, _ = dec.run(ckv, B, 256, 24)
        plain = plain[:B, :done2 + 1].cpu()
    lg = logits[:done].transpose(0, 1).cpu()
    masked = lg.clone()
    masked[..., ban] = float("-inf")
    am = masked.argmax(-1)
    emitted = toks[:, 1:]
    eos = cfg["eos_token_id"]
    for b in range(B):
        e = (emitted[b] == eos).nonzero()
        n = int(e[0]) + 1 if len(e) else emitted.shape[1]
        assert (emitted[b, :n] == am[b, :n]).all(), b
        assert (emitted[b, n:] == cfg["pad_token_id"]).all()
    assert not np.isin(emitted.numpy(), ban).any()
    assert (plain[:, 1:] == NAN_ROW).all()          # without the ban the NaN logit wins, as torch.argmax


def test_greedy_generate_beam_equals_generate_and_bans_hold(dev):
    from mrmt3.decode import generate, generate_beam
    m = _model("t5", torch.bfloat16, dev)
    _edit(m, _boost_eos)
    mel, _ = _enc(m, 3, seed=23)
    a = generate(m, mel, max_length=40)
    b = generate_beam(m, mel, num_beams=1, max_length=40, bad_token_ids=[])
    assert a.shape == b.shape and torch.equal(a, b)
    ban = sorted(set(a[:, 1:].flatten().tolist()) - {0, 1})[:40]
    c = generate_beam(m, mel, num_beams=1, max_length=40, bad_token_ids=ban)
    assert not np.isin(c.cpu().numpy(), ban).any() and not torch.equal(a, c)
    e = generate_beam(m, mel, num_beams=4, max_length=40, length_penalty=0.4, bad_token_ids=ban)
    assert not np.isin(e.cpu().numpy(), ban).any()
    assert e[:, 0].eq(0).all() and e.shape[1] <= 41


def test_songs_lockstep_equals_each_recording_alone(dev):
    """(d) one beam group per recording in lockstep = generate_beam per recording, bit for bit (fp32: the gemv step at
    any row count); the second segment of a recording takes its memory from the first one's best hypothesis."""
    from mrmt3.decode import _decoder_for, _memory, _memory_rows, generate_beam, generate_songs
    from mrmt3.synthetic import synth_mel
    m = _model("segmem_v2_with_prev", torch.float32, dev)
    _edit(m, _boost_eos)
    songs = [torch.from_numpy(synth_mel(n, frames=256, seed=40 + n)).to(dev) for n in (2, 1, 2)]
    ML, k = 32, 4
    lock = generate_songs(m, songs, max_length=ML, num_beams=k, length_penalty=0.4)
    alone = [generate_beam(m, s, num_beams=k, max_length=ML, length_penalty=0.4) for s in songs]
    for s, (a, b) in enumerate(zip(lock, alone)):
        assert a.shape == b.shape == (songs[s].shape[0], ML) and torch.equal(a, b), s
    eng, d, Lc = m.engine, m.cfg["d_model"], 256 + min(64, ML)
    with torch.no_grad():
        enc = eng.encode(songs[0]).view(2, 256, d)
        mem = _memory(eng, alone[0][0:1].contiguous(), 1, ML, Lc - 256)
        cur = torch.cat([enc[1:2], mem], 1).contiguous().view(Lc, d)
        dec = _decoder_for(m, k, ML, Lc)
        ids, _, _ = dec.run_beam(dec.cross_kv_beam(cur, 1, k, Lc), 1, k, Lc, ML, 0.4)
        assert torch.equal(_memory_rows(ids, ML)[0], alone[0][1])


def test_beam_graph_reuse_and_mode_switches(dev):
    """(e) the beam step replays a captured graph; two runs on one handle agree bit for bit; greedy -> beam -> greedy
    on one handle gives the first greedy ids back."""
    from mrmt3.decode import Decoder
    m = _model("t5", torch.bfloat16, dev)
    _edit(m, _boost_eos)
    d = m.cfg["d_model"]
    _, enc = _enc(m, 4, seed=31)
    dec = Decoder(m, 16, 32, 256)
    with torch.no_grad():
        ckv_g = dec.cross_kv(enc.reshape(4 * 256, d).contiguous(), 4, 256)
        g1, n1, _ = dec.run(ckv_g, 4, 256, 32)
        g1 = g1[:4, :n1 + 1].clone()
        ckv_b = dec.cross_kv_beam(enc.reshape(4 * 256, d).contiguous(), 4, 4, 256)
        b1 = dec.run_beam(ckv_b, 4, 4, 256, 32, 0.4)[0].clone()
        assert dec.graph_captured
        b2 = dec.run_beam(ckv_b, 4, 4, 256, 32, 0.4)[0].clone()
        ckv_g = dec.cross_kv(enc.reshape(4 * 256, d).contiguous(), 4, 256)
        g2, n2, _ = dec.run(ckv_g, 4, 256, 32)
        g2 = g2[:4, :n2 + 1].clone()
    assert torch.equal(b1, b2)
    assert torch.equal(g1, g2)


def test_beam_full_length_fills_the_cache(dev):
    """(e) k = 4, 1024 steps, no EOS: every position of the KV cache is written and reordered; the final rows' histories
    still reproduce the fp64 logits at every step."""
    m = _model("t5", torch.float32, dev)
    _edit(m, _no_eos)
    r = _beam(m, 1, 4, 1024, seed=3, lp=0.4)
    assert r.done == 1024 and r.fin == -1 and r.ids.shape == (1, 1025)
    assert not (r.bp[:, :, 1] == 1).any() and (r.bp[:, :, 0] >= 0).all() and (r.bp[:, :, 0] < 4).all()
    ref = BeamRef(1, 4, m.cfg["vocab_size"], length_penalty=0.4)
    ref.bp = [(r.bp[t, :, 0].numpy(), r.bp[t, :, 1].numpy()) for t in range(1024)]
    _check_cache(m, r, ref, 1024)


def test_beam_nan_logit_terminates_in_range(dev):
    m = _model("t5", torch.bfloat16, dev)
    _edit(m, _nan_row)
    r = _beam(m, 2, 4, 16, seed=5)
    assert r.done == 16 and r.fin == -1
    par, tok = r.bp[..., 0], r.bp[..., 1]
    group = torch.arange(8) // 4
    assert ((par // 4) == group).all() and (tok >= 0).all() and (tok < m.cfg["vocab_size"]).all()
    # every score is NaN: candidates rank by index, so EOS (index 1) is an early hypothesis; any width is legal
    assert r.ids.shape[1] <= 17 and (r.ids >= 0).all() and (r.ids < m.cfg["vocab_size"]).all()


def test_generate_beam_matches_an_fp64_cpu_beam_search(dev):
    """(f) two segments, k = 3, 24 new tokens: the fp32 handle and a float64 search over oracle.t5_ref (every step
    recomputed from the rows' full sequences) give the same ids."""
    from mrmt3.decode import generate_beam
    from mrmt3.synthetic import golden_weights
    from oracle import t5_ref
    m = _model("t5", torch.float32, dev)
    cfg, L = m.cfg, m.cfg["num_decoder_layers"]
    mel, _ = _enc(m, 2, seed=61)
    got = generate_beam(m, mel, num_beams=3, max_length=24, length_penalty=0.4).cpu()
    sd = {k: torch.from_numpy(v).double() for k, v in golden_weights(cfg, 0).items()}
    with torch.no_grad():
        enc = t5_ref.encode(sd, cfg, mel.double().cpu()).repeat_interleave(3, 0)
        ck = [enc @ sd[f"decoder.block.{i}.layer.1.EncDecAttention.k.weight"].t() for i in range(L)]
        cv = [enc @ sd[f"decoder.block.{i}.layer.1.EncDecAttention.v.weight"].t() for i in range(L)]

        def logits_fn(t, ids):
            return t5_ref.decode_step_logits(sd, cfg, torch.from_numpy(ids), ck, cv)[:, t].numpy()

        want, ref = beam_search(logits_fn, 2, 3, cfg["vocab_size"], 24, length_penalty=0.4)
    print(f"[f] smallest rank gap {min(ref.margins):.3e}")
    assert got.shape == want.shape and (got.numpy() == want).all(), (got, want)


def test_beam_decode_batches_of_different_widths_are_padded_and_stacked(dev):
    """5 segments, k = 4, room for 8 rows: `generate_beam` decodes 2 + 2 + 1 segments.  Its output is the three batches decoded
    by calls of their own, stacked to the widest: ids padded with pad_token_id, log-probabilities with 0.0, bit for bit.  EOS
    is made the twin of a token the last segment emits early, so its batch is narrower than the others (two layers, fp32)."""
    import mrmt3.decode as dec_mod
    from mrmt3.decode import generate_beam
    from mrmt3.synthetic import T5_SMALL
    from models.t5 import T5ForConditionalGeneration
    m = T5ForConditionalGeneration(dict(T5_SMALL, num_layers=2, num_decoder_layers=2), compute_dtype=torch.float32)
    m = m.load_golden().to(dev).eval()
    _edit(m, _no_eos)
    mel, _ = _enc(m, 5, seed=7, frames=16)
    kw = dict(num_beams=4, max_length=24, length_penalty=0.4, return_logprobs=True)
    old = dec_mod.MAX_DECODE_BATCH
    try:
        dec_mod.MAX_DECODE_BATCH = 8
        m._decoder = None
        tok = int(generate_beam(m, mel, num_beams=4, max_length=24)[4, 3])
        _edit(m, lambda w: w[1].copy_(w[tok] * 1.001))               # where `tok` would win, EOS now does, by a margin
        ids, lp = generate_beam(m, mel, **kw)
        parts = [generate_beam(m, mel[a:b], **kw) for a, b in ((0, 2), (2, 4), (4, 5))]
    finally:
        dec_mod.MAX_DECODE_BATCH = old
        m._decoder = None
    widths = [p[0].shape[1] for p in parts]
    print(f"[beam across batches] EOS = twin of {tok}; widths {widths}")
    assert len(set(widths)) > 1, widths                              # or nothing is padded and the test says nothing
    W, pad = max(widths), m.cfg["pad_token_id"]
    want = torch.cat([torch.nn.functional.pad(i, (0, W - i.shape[1]), value=pad) for i, _ in parts])
    want_lp = torch.cat([torch.nn.functional.pad(l, (0, W - l.shape[1]), value=0.0) for _, l in parts])
    assert ids.shape == (5, W) and torch.equal(ids, want)
    assert lp.dtype == torch.float32 and torch.equal(lp.view(torch.int32), want_lp.view(torch.int32))
