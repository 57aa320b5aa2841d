"""Sampled decoding on the GPU: the rule alone (`mrmt3_sample_logits`) against the host restatement
`tests/sample_ref.py`, then the sampled tail `dec_sample` through the decoder, the model calls and `InferenceHandler`.

A token is right when the host keeps it and its interval of the normalised cumulative probability holds the row's `u` within
SLACK = 2e-5 (the bound DESIGN §4e puts on the f32 sums of these rows; the kernel sums in f64, so the slack should never be
needed: at most 1 % of a case's tokens may be "decided by slack").  The standalone cases' seeds keep every `u` further than
SLACK from every edge (tests/test_sample_cpu.py), so there the kernel must return the host's token for every row.
Helpers are copies of tests/test_logprobs_gpu.py's (not imported)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LOGP_TOL = 2e-5
MAX_LOGIT = 64.0
STEPS = 24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- the rule alone ------------------------------------------------------------------------------------------------
def _ban_mask(ban, V, dev):
    if ban is None:
        return None
    m = torch.zeros(V, dtype=torch.uint8)
    m[list(ban)] = 1
    return m.to(dev)


def _ref_logp_np(lg, ban, tok):
    x = torch.from_numpy(lg).double()
    if ban is not None:
        x[:, list(ban)] = float("-inf")
    return torch.log_softmax(x, -1).gather(-1, torch.from_numpy(np.asarray(tok))[:, None]).squeeze(-1).numpy()


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_sample_logits_returns_the_host_token(dev, case):
    from mrmt3 import lib
    name, V, rows, kind, ban, T, k, p, seed = case
    lg = R.case_logits(name, V, rows, kind)
    ref = R.sample_ref(lg, ban, T, k, p)
    u = R.uniform(seed, R.CASE_ROW0 + np.arange(rows), R.CASE_STEP)
    tok, lp = lib.sample_logits(torch.from_numpy(lg).to(dev), T, k, p, seed, R.CASE_STEP, R.CASE_ROW0, _ban_mask(ban, V, dev),
                                return_logprobs=True)
    plain = lib.sample_logits(torch.from_numpy(lg).to(dev), T, k, p, seed, R.CASE_STEP, R.CASE_ROW0, _ban_mask(ban, V, dev))
    tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
    assert ((tok >= 0) & (tok < V)).all() and np.array_equal(plain.cpu().numpy(), tok)
    wrong, slack = ref.check(tok, u)
    same = tok == ref.pick(u)
    err = float(np.abs(lp - _ref_logp_np(lg, ban, tok)).max())
    print(f"[{name}] {rows} rows: {int(wrong.sum())} wrong, {int(slack.sum())} decided by slack, {int((~same).sum())} differ from "
          f"the host's token, {len(np.unique(tok))} distinct tokens, max kept {int(ref.kept.sum(1).max())}, max|logp - fp64| {err:.3e}")
    assert not wrong.any(), np.flatnonzero(wrong)[:8]
    assert slack.mean() <= 0.01
    assert same.all(), np.flatnonzero(~same)[:8]
    assert err <= LOGP_TOL                                           # whatever T and the filters are
    if ban is not None:
        assert not np.isin(tok, list(ban)).any()


def test_top_k_1_and_a_tiny_top_p_are_the_argmax(dev):
    """A unique maximum is returned whatever `u` is; a tied maximum is a tie group, kept whole by both filters (§4f), so
    there the draw must land on one of its members."""
    from mrmt3 import lib
    n_tied = 0
    for name, V, rows, kind in (("a", 1536, 9, "gauss"), ("b", 65, 4096, "gauss"), ("c", 64, 9, "ties"), ("d", 1536, 8, "ties"),
                                ("e", 5, 8, "ties"), ("f", 2048, 8, "live8")):
        lg = R.case_logits(name, V, rows, kind)
        x = torch.from_numpy(lg).to(dev)
        want = torch.argmax(x, -1).cpu().numpy()
        unique = (lg == lg.max(1, keepdims=True)).sum(1) == 1
        n_tied += int((~unique).sum())
        for kw in (dict(top_k=1), dict(top_p=1e-6), dict(top_k=1, temperature=0.5), dict(top_p=1e-6, temperature=2.0)):
            tok = lib.sample_logits(x, seed=77, step=3, **kw).cpu().numpy()
            assert np.array_equal(tok[unique], want[unique]), (name, kw)
            assert (lg[np.arange(rows), tok] == lg.max(1)).all(), (name, kw)
    assert n_tied > 0                                                # the tie rows do tie at the top


def test_vocabulary_beyond_the_registers_is_an_error_not_a_launch(dev):
    from mrmt3 import lib
    x = torch.zeros(2, 2049, device=dev)
    with pytest.raises(RuntimeError, match="2048"):
        lib.sample_logits(x)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5)):
        with pytest.raises(RuntimeError):
            lib.sample_logits(x[:, :64].contiguous(), **bad)
    torch.cuda.synchronize()
    assert lib.sample_logits(x[:, :2048].contiguous(), seed=1).shape == (2,)


def test_rows_without_a_distribution_emit_the_greedy_token(dev):
    from mrmt3 import lib
    V = 1536
    lg = R.case_logits("n", V, 9, "gauss")
    lg[1, 700] = np.nan
    lg[1, 900] = np.nan
    lg[4, :] = -np.inf
    lg[6, 33] = np.inf
    x = torch.from_numpy(lg).to(dev)
    tok, lp = lib.sample_logits(x, 1.0, 7, 0.9, seed=5, return_logprobs=True)
    tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
    ref = R.sample_ref(lg, None, 1.0, 7, 0.9)
    assert ref.greedy.tolist() == [r in (1, 4, 6) for r in range(9)]
    assert tok[[1, 4, 6]].tolist() == [700, 0, 33] and np.array_equal(tok[[1, 4, 6]], torch.argmax(x, -1).cpu().numpy()[[1, 4, 6]])
    assert np.isnan(lp[1]) and ((tok >= 0) & (tok < V)).all()
    wrong, _ = ref.check(tok, R.uniform(5, np.arange(9), 0))
    assert not wrong.any()
    # every token banned: the greedy token of an all -inf row, index 0; the NaNs banned away: a draw again
    tok = lib.sample_logits(x, seed=5, ban=torch.ones(V, dtype=torch.uint8, device=dev)).cpu().numpy()
    assert (tok == 0).all()
    ban = [700, 900]
    tok = lib.sample_logits(x, 1.0, 7, 0.9, seed=5, ban=_ban_mask(ban, V, dev)).cpu().numpy()
    ref = R.sample_ref(lg, ban, 1.0, 7, 0.9)
    assert not ref.greedy[1] and not ref.check(tok, R.uniform(5, np.arange(9), 0))[0].any()


# ---- through the decoder -------------------------------------------------------------------------------------------
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


def _edit(m, lm_edit):
    if lm_edit is not None:
        with torch.no_grad():
            lm_edit(m.flat.master("lm_head.weight"))
    m.engine.prepare(False)


def _twin_eos(m, ids, start):
    """lm_head row 1 (EOS) becomes 1.001 times the row of a token row `ids` emits at position `start` or later (its newest
    token otherwise): where that token wins with a positive logit EOS now wins instead, by a margin and not by a tie (an
    exact twin would tie at the top, and a tied maximum is a tie group that top_k = 1 keeps whole), so greedy ends that row
    there, some steps into the decode, and EOS carries about that token's probability when sampling."""
    seq = ids.tolist()
    cand = [t for t in dict.fromkeys(seq[1:]) if t > 1]
    late = [t for t in cand if seq.index(t, 1) >= start]
    tok = int(late[0] if late else cand[-1])
    _edit(m, lambda w: w[1].copy_(w[tok] * 1.001))
    return tok


def _enc(m, B, seed, frames=256):
    from mrmt3.synthetic import synth_mel
    mel = torch.from_numpy(synth_mel(B, frames=frames, seed=seed)).to(m.device)
    with torch.no_grad():
        return mel, m.engine.encode(mel).view(B, frames, m.cfg["d_model"])


def _live_mask(ids, eos):
    emitted = ids[:, 1:]
    after = torch.cumsum((emitted == eos).long(), -1) - (emitted == eos).long()
    return after == 0


def _run(m, dec, ckv, B, steps, sampling=None, ban=None, logprobs=False, dump=False, Lc=256):
    V = m.cfg["vocab_size"]
    with torch.no_grad():
        logits = torch.full((steps, B, V), float("nan"), device=m.device) if dump else None
        out = dec.run(ckv, B, Lc, steps, logits_out=logits, ban=dec.ban_mask(ban), return_logprobs=logprobs, sampling=sampling)
        assert dec.graph_captured
        torch.cuda.synchronize()
    done = out[1]
    ids = out[0][:B, :done + 1].cpu()
    lp = out[3][:B, :done + 1].cpu() if logprobs else None
    lg = logits[:done].transpose(0, 1).cpu() if dump else None       # [B, done, V]
    return ids, lp, lg


def _check_draws(ids, lg, eos, sp, ban=None, row_of=None, what=""):
    """Every live token of ids [B, 1 + T] against the host rule on that step's recorded logits lg [B, T, V]; row b draws
    with the counter (row_of[b], t)."""
    B, T, V = lg.shape
    live = _live_mask(ids, eos).numpy().reshape(-1)
    rows = np.repeat(np.arange(B) if row_of is None else np.asarray(row_of), T)
    steps = np.tile(np.arange(T), B)
    ref = R.sample_ref(lg.reshape(B * T, V).numpy(), ban, sp.temperature, sp.top_k, sp.top_p)
    u = R.uniform(sp.seed, rows, steps)
    wrong, slack = ref.check(ids[:, 1:].reshape(-1).numpy(), u)
    print(f"[{what}] {int(live.sum())} live tokens: {int(wrong[live].sum())} wrong, {int(slack[live].sum())} decided by slack, "
          f"kept per row {int(ref.kept.sum(1).min())}..{int(ref.kept.sum(1).max())}")
    assert not wrong[live].any(), np.flatnonzero(wrong & live)[:8]
    assert slack[live].mean() <= 0.01
    return live.reshape(B, T)


DEC = [(dt, B) for dt in (torch.float32, torch.bfloat16) for B in (3, 9)]


@pytest.mark.parametrize("dtype,B", DEC, ids=[f"{'fp32' if dt == torch.float32 else 'bf16'}-b{B}" for dt, B in DEC])
def test_decoder_draws_follow_the_rule_on_each_steps_logits(dev, dtype, B):
    from mrmt3.decode import Decoder, Sampling
    m = _model("t5", dtype, dev)
    _edit(m, None)
    eos, pad, d = m.cfg["eos_token_id"], m.cfg["pad_token_id"], m.cfg["d_model"]
    _, enc = _enc(m, B, seed=13 + B)
    dec = Decoder(m, B, STEPS, 256)
    with torch.no_grad():
        ckv = dec.cross_kv(enc.reshape(B * 256, d).contiguous(), B, 256)
    first, _, _ = _run(m, dec, ckv, B, STEPS)
    _twin_eos(m, first[0], 8)                                        # greedy row 0 now ends at step 7 or later
    greedy, _, _ = _run(m, dec, ckv, B, STEPS)
    n_cap = dec.capture_count
    again, _, _ = _run(m, dec, ckv, B, STEPS)
    assert torch.equal(again, greedy) and dec.capture_count == n_cap  # the plain capture is reused
    # top_k = 1 is the greedy decode through the sampled tail: finished rows emit pad, the others run on
    sp1 = Sampling(temperature=0.5, top_k=1, seed=3)
    one, _, _ = _run(m, dec, ckv, B, STEPS, sampling=sp1)
    assert dec.capture_count == n_cap + 1                            # sampling on: another tail, one capture
    assert torch.equal(one, greedy)
    glive = _live_mask(greedy, eos)
    assert (~glive).any() and (one[:, 1:][~glive] == pad).all()
    # a real draw: step by step with the logits recorded, then replayed from the graph
    sp = Sampling(temperature=1.0, top_k=0, top_p=0.9, seed=2024 + B)
    ids, lp, lg = _run(m, dec, ckv, B, STEPS, sampling=sp, logprobs=True, dump=True)
    assert float(lg.abs().max()) < MAX_LOGIT
    live = _check_draws(ids, lg, eos, sp, what=f"decoder {dtype} B={B}")
    live = torch.from_numpy(live)
    assert (ids[:, 1:][~live] == pad).all() and (lp[:, 1:][~live] == 0).all() and (lp[:, 0] == 0).all()
    ref_lp = torch.log_softmax(lg.double(), -1).gather(-1, ids[:, 1:, None]).squeeze(-1)
    err = float((lp[:, 1:].double() - ref_lp)[live].abs().max())
    print(f"[decoder {dtype} B={B}] max|logp - fp64| {err:.3e}; {int((ids != greedy).sum())} tokens differ from greedy")
    assert err <= LOGP_TOL                                           # the model's own confidence: before T and the filters
    n_cap = dec.capture_count
    rep, rep_lp, _ = _run(m, dec, ckv, B, STEPS, sampling=sp, logprobs=True)
    assert torch.equal(rep, ids) and torch.equal(rep_lp, lp)         # graph replay == step by step, bit for bit
    assert dec.capture_count == n_cap                                # (step by step replays the same captured step)
    other, _, lg2 = _run(m, dec, ckv, B, STEPS, sampling=Sampling(1.0, 0, 0.9, seed=sp.seed + 1), logprobs=True, dump=True)
    assert other.shape != ids.shape or not torch.equal(other, ids)   # another seed, another transcription
    _check_draws(other, lg2, eos, Sampling(1.0, 0, 0.9, seed=sp.seed + 1), what="other seed")
    hot = Sampling(2.0, 7, 1.0, seed=sp.seed)
    ids3, _, lg3 = _run(m, dec, ckv, B, STEPS, sampling=hot, logprobs=True, dump=True)
    _check_draws(ids3, lg3, eos, hot, what="T=2 k=7")
    assert dec.capture_count == n_cap and dec.graph_captured          # new seed, new parameters: no re-capture
    back, _, _ = _run(m, dec, ckv, B, STEPS)
    assert torch.equal(back, greedy)                                 # and the plain decode is what it was


def test_sampling_with_a_ban_and_without_logprobs(dev):
    from mrmt3.decode import Decoder, Sampling
    B, ban = 4, list(range(2, 700, 3))
    m = _model("t5", torch.bfloat16, dev)
    _edit(m, None)
    _, enc = _enc(m, B, seed=31)
    dec = Decoder(m, B, STEPS, 256)
    with torch.no_grad():
        ckv = dec.cross_kv(enc.reshape(B * 256, m.cfg["d_model"]).contiguous(), B, 256)
    sp = Sampling(0.5, 0, 0.9, seed=8)
    ids, _, lg = _run(m, dec, ckv, B, STEPS, sampling=sp, ban=ban, dump=True)
    _check_draws(ids, lg, m.cfg["eos_token_id"], sp, ban=ban, what="ban")
    assert not np.isin(ids[:, 1:].numpy(), ban).any()
    with_lp, _, _ = _run(m, dec, ckv, B, STEPS, sampling=sp, ban=ban, logprobs=True)
    assert torch.equal(with_lp, ids)


def test_beam_search_refuses_sampling(dev):
    import ctypes as C
    from mrmt3 import lib
    from mrmt3.decode import Decoder
    m = _model("t5", torch.bfloat16, dev)
    _edit(m, None)
    _, enc = _enc(m, 2, seed=3)
    dec = Decoder(m, 4, 8, 256)
    with torch.no_grad():
        ckv = dec.cross_kv_beam(enc.reshape(2 * 256, m.cfg["d_model"]).contiguous(), 2, 2, 256)
        with torch.cuda.stream(dec.stream):
            dec.begin_beam(ckv, 2, 2, 256)
            rc = lib.load().mrmt3_decoder_set_sampling(dec.h, 1.0, 0, 1.0, 0, lib._stream())
            assert rc != 0 and b"beam" in lib.load().mrmt3_last_error()
            for bad in ((-1.0, 0, 1.0), (float("nan"), 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.5)):
                assert lib.load().mrmt3_decoder_set_sampling(dec.h, *bad, 0, lib._stream()) != 0
        torch.cuda.synchronize()


def test_scores_of_sampled_tokens_match_model_score(dev):
    """The bound of tests/test_logprobs_gpu.py's greedy cross-check: twice the largest logit difference between the training
    forward and the decode step at the scored positions, plus LOGP_TOL."""
    from mrmt3.decode import generate_sample
    B = 3
    m = _model("t5", torch.float32, dev)
    _edit(m, None)
    mel, enc = _enc(m, B, seed=43)
    ids, lp = generate_sample(m, mel, max_length=STEPS, temperature=1.0, top_p=0.9, seed=17, return_logprobs=True)
    ids, lp = ids.cpu(), lp.cpu()
    live = _live_mask(ids, m.cfg["eos_token_id"])
    labels = torch.where(live, ids[:, 1:], torch.full_like(ids[:, 1:], -100)).to(dev).contiguous()
    with torch.no_grad():
        sc = m.score(mel, labels).cpu()
        fwd = m(inputs=mel, labels=labels).cpu()
    # the decode step's logits, recorded on a second, identical run
    dec = m._decoder
    with torch.no_grad():
        ckv = dec.cross_kv(enc.reshape(B * 256, m.cfg["d_model"]).contiguous(), B, 256)
    from mrmt3.decode import Sampling
    ids2, _, lg = _run(m, dec, ckv, B, ids.shape[1] - 1, sampling=Sampling(1.0, 0, 0.9, 17), logprobs=True, dump=True)
    assert torch.equal(ids2, ids)
    gap = float((fwd.double() - lg.double()).abs().max(-1).values[live].max())
    diff = float((sc.double() - lp[:, 1:].double())[live].abs().max())
    print(f"[sample vs score] max|forward logits - decode logits| {gap:.3e}; max|score - decoder logp| {diff:.3e} over "
          f"{int(live.sum())} tokens")
    assert int(live.sum()) > B
    assert diff <= 2 * gap + LOGP_TOL, (diff, gap)


def test_several_samples_per_segment_and_best_of(dev):
    from mrmt3.decode import Decoder, Sampling, generate_best_of, generate_sample
    G, n = 2, 3
    m = _model("t5", torch.bfloat16, dev)
    _edit(m, None)
    eos, d = m.cfg["eos_token_id"], m.cfg["d_model"]
    mel, enc = _enc(m, G, seed=29)
    kw = dict(max_length=STEPS, temperature=1.0, top_k=0, top_p=0.95, seed=5)
    ids, lp = generate_sample(m, mel, num_return_sequences=n, return_logprobs=True, **kw)
    assert ids.shape[0] == G * n and lp.shape == ids.shape
    for g in range(G):
        rows = [ids[g * n + j].tolist() for j in range(n)]
        assert len({tuple(r) for r in rows}) == n, rows              # the samples of a segment differ from each other
    # rows of a plain decode are single-sample decodes: row g * n + j, fed segment g's K|V, draws with the counter g * n + j
    dec = Decoder(m, G * n, STEPS, 256)
    with torch.no_grad():
        ckv = dec.cross_kv_beam(enc.reshape(G * 256, d).contiguous(), G, n, 256)
    sp = Sampling(1.0, 0, 0.95, 5)
    one, one_lp, lg = _run(m, dec, ckv, G * n, STEPS, sampling=sp, logprobs=True, dump=True)
    w = ids.shape[1]                                                 # `generate_sample` cuts after the step every row is done
    assert torch.equal(one[:, :w], ids.cpu()) and bool((one[:, w:] == m.cfg["pad_token_id"]).all())
    _check_draws(one, lg, eos, sp, what="n=3")
    # ... and a segment decoded alone at another row draws another stream
    alone = generate_sample(m, mel[1:2], **kw)
    assert alone.shape != ids[n:n + 1].shape or not torch.equal(alone, ids[n:n + 1])
    best, best_lp = generate_best_of(m, mel, n, **kw)
    live = _live_mask(ids.cpu(), eos)
    score = torch.where(live, lp.cpu()[:, 1:].double(), torch.zeros((), dtype=torch.float64)).sum(-1).view(G, n)
    for g in range(G):
        j = max(range(n), key=lambda j: (float(score[g, j]), -j))
        assert torch.equal(best[g].cpu(), ids[g * n + j].cpu()) and torch.equal(best_lp[g].cpu(), lp[g * n + j].cpu()), (g, j)
    print(f"[best of {n}] scores {score.tolist()}")
    with pytest.raises(ValueError):
        m.generate_beam(mel, num_beams=2, do_sample=True)


def test_memory_models_carry_their_sampled_tokens(dev):
    """V2WithPrev: segment i draws with seed + i at row 0 and its memory ids are segment i - 1's sampled tokens;
    `generate_2`: the prefix steps draw nothing, token step t draws with the counter (0, t)."""
    from mrmt3.decode import Decoder, Sampling, generate, generate_2, _memory
    ML = STEPS
    m = _model("segmem_v2_with_prev", torch.float32, dev)
    _edit(m, None)
    eng, d, eos = m.engine, m.cfg["d_model"], m.cfg["eos_token_id"]
    mel, enc = _enc(m, 2, seed=61)
    sp = Sampling(1.0, 0, 0.9, seed=40)
    ids = generate(m, mel, max_length=ML, do_sample=True, top_p=0.9, seed=40)
    assert ids.shape == (2, ML) and torch.equal(ids, m.generate_sample(mel, max_length=ML, top_p=0.9, seed=40))
    assert not torch.equal(ids, generate(m, mel, max_length=ML))
    Ls = min(m.segmem_length, ML)
    dec = Decoder(m, 1, ML, 256 + Ls)
    prev = torch.zeros(1, ML, dtype=torch.int64, device=dev)
    prev[0, 0], prev[0, 1] = 1134, 1
    for i in range(2):
        with torch.no_grad():
            mem = _memory(eng, prev, 1, ML, Ls)
            cur = torch.cat([enc[i:i + 1], mem], 1).contiguous().view(256 + Ls, d)
            ckv = dec.cross_kv(cur, 1, 256 + Ls)
        one, _, lg = _run(m, dec, ckv, 1, ML, sampling=sp.shifted(i), dump=True, Lc=256 + Ls)
        _check_draws(one, lg, eos, sp.shifted(i), what=f"v2 segment {i}")
        w = min(one.shape[1], ML)
        assert torch.equal(one[0, :w], ids[i, :w].cpu()), i          # fed the SAMPLED segment i - 1, it reproduces segment i
        prev = ids[i:i + 1].clone()
    m1 = _model("segmem_v1", torch.float32, dev)
    _edit(m1, None)
    mel1, _ = _enc(m1, 2, seed=37)
    a = generate_2(m1, mel1, max_length=64, do_sample=True, temperature=0.5, top_k=7, seed=3)
    b, b_lp = generate_2(m1, mel1, max_length=64, do_sample=True, temperature=0.5, top_k=7, seed=3, return_logprobs=True)
    assert torch.equal(a, b) and a.shape == (2, 64) and bool((b_lp <= 0).all())
    assert not torch.equal(a, generate_2(m1, mel1, max_length=64))
    # segment 0 again on a handle of its own, logits recorded: 64 prefix steps, then token step t draws with (0, t)
    n_pre, steps = m1.segmem_length, 16
    sp2 = Sampling(0.5, 7, 1.0, 3)
    with torch.no_grad():
        enc1 = m1.engine.encode(mel1).view(2, 256, d)
        seg = torch.zeros(1, 64, dtype=torch.int64, device=dev)
        seg[0, 0] = 1
        pre = m1.engine.segmem(seg, 1, 64).float().view(1, n_pre, d).contiguous()
        dec1 = Decoder(m1, 1, n_pre + steps, 256)
        ckv = dec1.cross_kv(enc1[0].contiguous(), 1, 256)
        logits = torch.full((n_pre + steps, 1, m1.cfg["vocab_size"]), float("nan"), device=dev)
        toks, done, fin = dec1.run(ckv, 1, 256, steps, prefix=pre, logits_out=logits, sampling=sp2)
        torch.cuda.synchronize()
    T = done - n_pre
    one = toks[:1, :T + 1].cpu()
    _check_draws(one, logits[n_pre:done].transpose(0, 1).cpu(), eos, sp2, what="generate_2 segment 0")
    assert torch.equal(one[0, :T + 1], a[0, :T + 1].cpu())


def test_inference_handler_samples_only_under_decode_options(dev):
    import inference
    from mrmt3.synthetic import synth_audio
    m = _model("t5", torch.float32, dev)
    _edit(m, None)
    audio = synth_audio(1, n_samples=3 * 32768, seed=9)[0]
    off = inference.InferenceHandler(model=m, device=dev, decode_options=False)
    plain, _ = off.inference(audio, max_length=32, return_tokens=True)
    same, _ = off.inference(audio, max_length=32, return_tokens=True, do_sample=True, temperature=2.0, seed=4, best_of=2)
    assert all(np.array_equal(a, b) for a, b in zip(plain, same))    # the keywords change nothing
    on = inference.InferenceHandler(model=m, device=dev, decode_options=True)
    kw = dict(max_length=32, do_sample=True, temperature=1.5, top_p=0.95, seed=4)
    a, _ = on.inference(audio, return_tokens=True, **kw)
    b, _ = on.inference(audio, return_tokens=True, **kw)
    c, _ = on.inference(audio, return_tokens=True, **dict(kw, seed=5))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not all(np.array_equal(x, y) for x, y in zip(a, plain)) and not all(np.array_equal(x, y) for x, y in zip(a, c))
    n1, n2 = on.inference(audio, **kw), on.inference(audio, **kw)
    assert n1.notes == n2.notes                                      # the same seed, the same notes
    scored = on.inference(audio, with_confidence=True, **kw)
    assert scored.notes == n1.notes and all(0.0 < n.confidence <= 1.0 for n in scored.notes)
    best, _, lps = on.inference(audio, return_tokens=True, with_confidence=True, best_of=3, batch_size=2, **kw)
    n_seg = sum(len(x) for x in plain)
    assert len(best) == (n_seg + 1) // 2 and all(t.shape == l.shape for t, l in zip(best, lps))
    many = on.inference_many([audio, audio[:32768]], return_tokens=True, **kw)
    assert len(many) == 2 and many[0][0][0].shape[0] == n_seg


def test_several_samples_per_segment_across_decode_batches(dev):
    """`num_return_sequences` = 4 with room for 8 rows: 3 segments decode as 2 + 1, batch c under `seed + c`, the batches padded
    to the widest and stacked.  Against `Decoder.run` driven by hand, bit for bit; row g * 4 + j is sample j of segment g."""
    import mrmt3.decode as dec_mod
    from mrmt3.decode import Decoder, Sampling, generate_sample
    from mrmt3.synthetic import T5_SMALL
    from models.t5 import T5ForConditionalGeneration
    G, n, Le, ML, seed = 3, 4, 16, STEPS, 5
    m = T5ForConditionalGeneration(dict(T5_SMALL, num_layers=2, num_decoder_layers=2), compute_dtype=torch.float32)
    m = m.load_golden().to(dev).eval()
    _edit(m, lambda w: w[1].mul_(3.5))                               # EOS is drawn now and then: the batches end at different steps
    pad, d = m.cfg["pad_token_id"], m.cfg["d_model"]
    mel, enc = _enc(m, G, seed=7, frames=Le)
    kw = dict(temperature=1.0, top_k=50, top_p=0.95)
    old = dec_mod.MAX_DECODE_BATCH
    try:
        dec_mod.MAX_DECODE_BATCH = 8
        m._decoder = None
        ids, lp = generate_sample(m, mel, max_length=ML, num_return_sequences=n, seed=seed, return_logprobs=True, **kw)
    finally:
        dec_mod.MAX_DECODE_BATCH = old
        m._decoder = None
    parts = []
    for c, (g0, ns) in enumerate(((0, 2), (2, 1))):
        dec = Decoder(m, ns * n, ML, Le)
        with torch.no_grad():
            ckv = dec.cross_kv_beam(enc[g0:g0 + ns].reshape(ns * Le, d).contiguous(), ns, n, Le)
            toks, _, fin, logp = dec.run(ckv, ns * n, Le, ML, sampling=Sampling(seed=seed + c, **kw), return_logprobs=True)
        w = 1 + (fin + 1 if fin >= 0 else ML)
        parts.append((toks[:ns * n, :w].clone(), logp[:ns * n, :w].clone()))
    W = max(t.shape[1] for t, _ in parts)
    print(f"[n=4 across batches] widths {[t.shape[1] for t, _ in parts]}")
    want = torch.cat([torch.nn.functional.pad(t, (0, W - t.shape[1]), value=pad) for t, _ in parts])
    want_lp = torch.cat([torch.nn.functional.pad(l, (0, W - l.shape[1]), value=0.0) for _, l in parts])
    assert ids.shape == (G * n, W) and torch.equal(ids, want)
    assert lp.dtype == torch.float32 and torch.equal(lp.view(torch.int32), want_lp.view(torch.int32))
