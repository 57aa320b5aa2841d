"""Element-exact tests of the decode tail (csrc/decode_tail.hip) on a real MI355X: tail probes with designed logits.

A tail probe (tests/_exact_tail.py, proven on the CPU by tests/test_exact_tail_cpu.py) is a one-layer handle driven through the C
ABI only (mrmt3_decoder_create / begin / begin_beam / set_ban / set_logprobs / set_sampling / run with one step at a time / logits
/ poll / beam_finalize_logprobs) that runs TOKEN steps: its logits are integers the host designs, as a function of (token taken,
position, row).  On a bf16 handle the copied logits of every step equal the design bit for bit, so the host derives the whole
decode by the documented rule and every token, log-probability, parent, score, hypothesis record and poll triple is asserted per
(row, step).  On an f32 handle (the gemv path, rows <= 8) the copy is within `lm_head_f32_bound` of the design, columns with
identical lm_head rows are asserted bit-equal and the rule is applied to the copy.  No assertion is a norm or a maximum over rows.
The reorder probes are two-layer handles whose logits also show the KV cache: (V[fresh] + V[old]) / 2 of the read layer.

Which test asserts which kernel instantiation's output (the dispatch follows from what was set on the handle: ban, log-probabilities,
sampling or beam mode are the captured step's key, `mrmt3_decoder_capture_count` is asserted to count each once and
`mrmt3_decoder_graph_captured` to be 1):
  dec_argmax<0, 0> <0, 1> <1, 0> <1, 1>   test_greedy_tail_on_designed_logits: V = 1536, 1491, 512, 65, 40 on f32 B = 3 and bf16
                                          B = 3, 8, 9, 17, V = 2048 (the register limit of LOGP) on bf16 B = 9; the open and the
                                          closed probe each; test_greedy_tail_on_rows_without_a_number (+-inf alone, every token
                                          banned); <0, 0> with 32 workgroups: test_greedy_state_of_256_rows
  dec_step_close, dec_emit_row            the same tests: the poll triple after every step, pads and their 0.0, the next logits
  dec_sample<0, 0> <0, 1> <1, 0> <1, 1>   test_sampled_tail_draws_with_the_counter_of_row_and_step (V = 1536 and 40, bf16 B = 9,
                                          f32 B = 3, two seeds on one captured step; the nine-row cases at V = 1536 keep the 40
                                          largest logits, so nine rows with all 1536 columns kept are NOT run: f32 B = 3 is the
                                          only handle that draws from the whole 1536-column row)
  dec_beam_select, dec_beam_begin_kernel, test_beam_search_on_designed_logits (k x groups = 1 x 1, 2 x 3, 3 x 3, 8 x 1, 8 x 2;
  dec_beam_finalize_kernel                V = 1536, 1491, 40, 2048; length penalty 1.0 and 0.4; static bans), test_beam_search_of_
                                          256_rows (8 x 32), test_beam_lds_limit_is_exact (k = 8: V = 2048 runs, V = 2049 is refused)
  dec_beam_reorder                        test_reorder_moves_every_slot_of_both_layers (two-layer probes, 28 steps, 3 groups of 3 and
                                          of 8 beams, bf16 at 768 and f32 at 1536 bytes a position, layer 1 and layer 0 read back),
                                          test_reorder_of_32_groups (256 rows)

Where the header was silent the reference is torch (`torch.argmax`, float64 `log_softmax`): a row of -inf alone, +inf beside
-inf, or every token banned emits token 0 with a NaN log-probability.  The f32 handle keeps every designed tie group bit-equal
(duplicate lm_head rows give duplicate columns); ties between columns whose lm_head rows differ exist on bf16 handles only.

Observed on an MI355X (`EXACT-TAIL` lines; the bounds come from the project's tolerances, never from these values):
  the file's wall time: 6.3 s (59 tests, 8.7 s with collection)
  greedy log-probability, largest error / LOGP_TOL over the four instantiations and both probes:
                f32-b3   bf16-b3  bf16-b8  bf16-b9  bf16-b17
    V = 1536    0.034    0.034    0.037    0.034    0.038
    V = 1491    0.033    0.028    0.036    0.029    0.040
    V = 512     0.014    0.015    0.024    0.019    0.018
    V = 65      0.011    0.012    0.014    0.014    0.011
    V = 40      0.007    0.009    0.011    0.012    0.013        V = 2048, bf16-b9: 0.044
  bf16 logits: 0 error against the design on every handle (bit-exact, NaN and +-inf included)
  beam search, largest score error (beam scores and hypothesis scores) / `_tol` of the largest score / smallest untied gap:
    k1-g1-v40-f32 2.6e-7 / 2.9e-5 / 4.0        k1-g1-v1491-ban-bf16 2.3e-7 / 5.0e-5 / 2.0      k2-g3-v1491-bf16 9.5e-7 / 6.3e-5 / 9.9e-2
    k2-g3-v1491-f32 1.4e-7 / 4.2e-5 / 2.0      k3-g3-v1536-bf16 3.1e-6 / 1.2e-4 / 2.3e-3       k3-g3-v40-ban-bf16 4.8e-7 / 4.7e-5 / 1.4e-2
    k8-g2-v1536-bf16 1.0e-6 / 6.6e-5 / 1.8e-3  k8-g1-v1491-ban-f32 9.8e-7 / 1.2e-4 / 1.8e-2    k2-g2-v40-nan-bf16 1.2e-6 / 5.3e-5 / 1.1e-2
    k8-g1-v2048-bf16 4.3e-7 / 4.9e-5 / 7.5e-3  k8-g32-v1536-bf16 1.9e-6 / 7.4e-5 / 1.3e-3
    the two eos-only cases hold hypotheses at -1e9 + log p: error 6.9 (bf16) and 29 (f32) of `_tol`(1e9) = 4000, gaps of 1e9
  reorder probes, largest read-out error / ATTN_TOL, score error, smallest gap: read1 (layer 1, unit 2.0) 0.000 on every handle,
    read0 bf16 0.054 (two bf16 roundings of the final norm; the CPU proof bounds them by 0.0625), read0 f32 0.000; score errors
    1.3e-6 to 4.0e-6; gaps 4.9e-4 (k = 8, 3 groups) to 3.5e-3
An f32 handle does NOT keep a tie between columns whose lm_head rows differ, nor between rows whose residuals differ in their
+-1 codes (sums of equal value round differently): the first f32 designs tied such candidates and their copies showed gaps of
2e-6 to 6e-6, neither 0 nor above the margin.  Nothing was loosened: the f32 designs now tie duplicate lm_head rows under one
residual only (`beam_design_f32`, `BeamEmu(strict=)`), which the device keeps bit-equal; every other tie scenario
runs on the bf16 handles.
"""
import ctypes as C
import functools
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact_decode as ed  # noqa: E402
import _exact_tail as et  # noqa: E402

pytestmark = pytest.mark.gpu

HANDLES = [("f32-b3", False, 3), ("bf16-b3", True, 3), ("bf16-b8", True, 8), ("bf16-b9-mfma", True, 9),
           ("bf16-b17-mfma", True, 17)]
BIG = ("bf16-b256-mfma", True, 256)
VOCABS = (1536, 1491, 512, 65, 40)
_ids = lambda hs: [h[0] for h in hs]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    t0 = time.time()
    yield torch.device("cuda:0")
    print("EXACT-TAIL wall %.1f s" % (time.time() - t0))


@functools.lru_cache(maxsize=64)
def greedy_probe(V, B, variant):
    """Built once and shared between the handles and the tail modes, never modified."""
    p = et.greedy_design(V, B, variant)
    et.check_tail_probe(p)
    return p


# ---- the handle ----------------------------------------------------------------------------------------------------------------------

class Handle:
    """One decoder handle over probe p on a stream of its own.  Everything the step graph bakes in is allocated here once."""

    def __init__(self, dev, p, bf16):
        from mrmt3 import lib
        from mrmt3.decode import _Weights
        self.lib, self.l, self.p, self.dev, self.bf16 = lib, lib.load(), p, dev, bf16
        dt = torch.bfloat16 if bf16 else torch.float32
        B, T, V = p.B, p.T, p.V
        self.max_len = T
        on = lambda t, d: t.to(device=dev, dtype=d).contiguous()
        dev_w = lambda w: {k: on(t, torch.float32 if k.startswith("ln_") or k == "final_ln" else dt) for k, t in w.items()}
        self.w = dev_w(p.w)                                          # lm_head and final_ln; a one-layer probe keeps its layer here too
        self.layers = [dev_w(w) for w in getattr(p, "layers", [p.w])]
        n_layers = len(self.layers)
        self.embed, self.pos = on(p.embed, torch.float32), on(p.pos, torch.float32)
        self.ckv = on(torch.cat([p.ck, p.cv], -1).view(n_layers, B, p.Lc, 2 * ed.INNER), dt)
        self.tokens = torch.zeros(B, T + 1, dtype=torch.int64, device=dev)
        self.ban = torch.zeros(V, dtype=torch.uint8, device=dev)
        self.logp = torch.zeros(B, T + 1, device=dev)
        self.out = torch.zeros(T, B, V, device=dev)
        self.pinned = torch.zeros(T, 3, dtype=torch.int32).pin_memory()
        names = ("ln_self", "w_qkv", "w_o_self", "ln_cross", "w_q_cross", "w_o_cross", "ln_ff", "w_wi", "w_wo")
        self.keep = {k: (C.c_void_p * n_layers)(*[w[k].data_ptr() for w in self.layers]) for k in names}
        self.ws = _Weights()
        self.ws.embed, self.ws.pos = self.embed.data_ptr(), self.pos.data_ptr()
        self.ws.lm_head, self.ws.final_ln = self.w["lm_head"].data_ptr(), self.w["final_ln"].data_ptr()
        for k, a in self.keep.items():
            setattr(self.ws, k, C.cast(a, C.POINTER(C.c_void_p)))
        self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream())
        self.h = C.c_void_p()
        lib._check(self.l.mrmt3_decoder_create(C.byref(self.h), n_layers, ed.D, ed.H, ed.DFF, V, B, self.max_len, p.Lc,
                                               lib.BF16 if bf16 else lib.F32, ed.EPS), "decoder_create")

    def close(self):
        self.l.mrmt3_decoder_destroy(self.h)

    def steps(self, T, after=None):
        """T replays, each followed by a copy of the logits and of the poll triple; no host synchronisation in between."""
        lib, l = self.lib, self.l
        for t in range(T):
            lib._check(l.mrmt3_decoder_run(self.h, 1, lib._stream()), "decoder_run")
            lib._check(l.mrmt3_decoder_logits(self.h, lib._p(self.out[t]), self.p.B, lib._stream()), "decoder_logits")
            lib._check(l.mrmt3_decoder_poll(self.h, C.c_void_p(self.pinned.data_ptr() + 12 * t), lib._stream()), "decoder_poll")
            if after is not None:
                after(t)

    def beam_buffers(self, G):
        """The caller-owned buffers of mrmt3_decoder_begin_beam, filled with values no search writes."""
        rows, T, dev = self.p.B, self.p.T, self.dev
        self.bp = torch.full((self.max_len, rows, 2), -9, dtype=torch.int32, device=dev)
        self.bscore = torch.full((rows,), 123.0, device=dev)
        self.hyp = torch.full((G, et.HREC), -9, dtype=torch.int32, device=dev)
        self.out_ids = torch.full((G, T + 1), -9, dtype=torch.int64, device=dev)
        self.out_logp = torch.full((G, T + 1), 123.0, device=dev)
        self.snap_scores = torch.zeros(T, rows, device=dev)
        self.snap_hyps = torch.zeros(T, G, et.HREC, dtype=torch.int32, device=dev)

    def begin_beam(self, k, G, lp, ban):
        lib, p = self.lib, self.p
        return self.l.mrmt3_decoder_begin_beam(self.h, C.byref(self.ws), lib._p(self.ckv), G, k, p.Lc, lib._p(self.tokens), et.START,
                                               et.EOS, et.PAD, float(lp), lib._p(self.ban) if ban is not None else None,
                                               lib._p(self.bp), lib._p(self.bscore), lib._p(self.hyp), lib._stream())

    def beam(self, k, G, lp, ban=None):
        """One beam search of p.T steps and its finalize: what every step and the finalize left in the caller's buffers."""
        lib, l, p = self.lib, self.l, self.p
        T = p.T
        self.beam_buffers(G)

        def snap(t):
            self.snap_scores[t].copy_(self.bscore)
            self.snap_hyps[t].copy_(self.hyp)

        with torch.cuda.stream(self.stream):
            if ban is not None:
                self.ban.copy_(torch.from_numpy(np.asarray(ban, dtype=np.uint8)))
            self.out.fill_(float("nan"))
            self.pinned.fill_(-7)
            lib._check(self.begin_beam(k, G, lp, ban), "decoder_begin_beam")
            self.steps(T, snap)
            lib._check(l.mrmt3_decoder_beam_finalize_logprobs(self.h, lib._p(self.out_ids), lib._p(self.out_logp), T + 1, T,
                                                              lib._stream()), "decoder_beam_finalize_logprobs")
        self.stream.synchronize()
        assert l.mrmt3_decoder_graph_captured(self.h) == 1 and l.mrmt3_decoder_capture_count(self.h) == 1
        return SimpleNamespace(bp=self.bp[:T].cpu(), tokens=self.tokens[:, 1:T + 1].cpu(), scores=self.snap_scores.cpu(),
                               hyps=self.snap_hyps.cpu(), polls=self.pinned[:T].clone(), ids=self.out_ids.cpu(),
                               out_logp=self.out_logp.cpu(), final_hyps=self.hyp.cpu(), logits=self.out[:T].transpose(0, 1).cpu())

    def greedy(self, ban=None, logp=False, sampling=None, T=None):
        """One greedy or sampled decode of T token steps -> tokens [B, T], logp [B, T], logits [B, T, V], polls [T, 3]."""
        lib, l, p = self.lib, self.l, self.p
        T = T or p.T
        with torch.cuda.stream(self.stream):
            if ban is not None:
                self.ban.copy_(torch.from_numpy(np.asarray(ban, dtype=np.uint8)))
            self.out.fill_(float("nan"))
            self.logp.fill_(float("nan"))
            self.pinned.fill_(-7)
            lib._check(l.mrmt3_decoder_begin(self.h, C.byref(self.ws), lib._p(self.ckv), p.B, p.Lc, lib._p(self.tokens), et.START,
                                             et.EOS, et.PAD, lib._stream()), "decoder_begin")
            if ban is not None:
                lib._check(l.mrmt3_decoder_set_ban(self.h, lib._p(self.ban), lib._stream()), "decoder_set_ban")
            if logp:
                lib._check(l.mrmt3_decoder_set_logprobs(self.h, lib._p(self.logp), T + 1, lib._stream()), "decoder_set_logprobs")
            if sampling is not None:
                seed, temp, top_k, top_p = sampling
                lib._check(l.mrmt3_decoder_set_sampling(self.h, float(temp), int(top_k), float(top_p), int(seed), lib._stream()),
                           "decoder_set_sampling")
            self.steps(T)
        self.stream.synchronize()
        assert l.mrmt3_decoder_graph_captured(self.h) == 1
        return SimpleNamespace(tokens=self.tokens[:, 1:T + 1].cpu(), logp=self.logp[:, 1:T + 1].cpu().double(),
                               logits=self.out[:T].transpose(0, 1).cpu(), polls=self.pinned[:T].clone(),
                               captures=l.mrmt3_decoder_capture_count(self.h), start=self.tokens[:, 0].cpu())


def check_logits(what, p, bf16, got, ref):
    """bf16: the copy IS the design.  f32: within the bound of the operation chain, identical lm_head rows bit-equal."""
    if bf16:
        et.check_equal(what + " logits", got.logits, ref.logits.float())
        return 0.0
    ratio = et.check_within(what + " logits", got.logits, ref.logits, et.f32_bound(p, ref.logits))
    bits = got.logits.contiguous().view(torch.int32)
    for g in et.identical_columns(p):
        ed.check_equal(what + " tie group %s" % g[:4], bits[..., g[1:]], bits[..., g[:1]].expand(-1, -1, len(g) - 1))
    return ratio


def check_greedy_run(what, p, bf16, got, ban, logp, sampling=None):
    """One decode against the rule: on the design (bf16) or on the copy (f32).  -> the reference trace."""
    assert bool((got.start == et.START).all())
    ref = et.greedy_trace(p, ban, sampling, copy=None if bf16 else got.logits, T=got.tokens.shape[1])
    ed.check_equal(what + " tokens", got.tokens[..., None], ref.tokens[..., None])       # first: the logits follow the tokens
    check_logits(what, p, bf16, got, ref)
    ref.ratio = et.check_greedy(what, got, ref, logp)              # largest log-probability error / LOGP_TOL
    return ref


# ---- a. the greedy tail: dec_argmax<BAN, LOGP> ---------------------------------------------------------------------------------------

GREEDY = [(h, V) for h in HANDLES for V in VOCABS] + [(HANDLES[3], 2048)]


@pytest.mark.parametrize("handle,V", GREEDY, ids=["%s-v%d" % (h[0], V) for h, V in GREEDY])
def test_greedy_tail_on_designed_logits(dev, handle, V):
    """The four dec_argmax<BAN, LOGP> on the open and the closed probe: every token, log-probability, poll triple and (through
    the next step's logits) next input."""
    tag, bf16, B = handle
    ban = et.greedy_ban(V)
    worst = 0.0
    for variant in ("open", "closed"):
        p = greedy_probe(V, B, variant)
        h = Handle(dev, p, bf16)
        try:
            n = 0
            for use_ban in (False, True):
                for logp in (False, True):
                    got = h.greedy(ban if use_ban else None, logp)
                    n += 1
                    assert got.captures == n                         # BAN and LOGP are part of the captured step's key
                    ref = check_greedy_run("greedy %s V=%d %s ban=%d logp=%d" % (tag, V, variant, use_ban, logp), p, bf16, got,
                                           ban if use_ban else None, logp)
                    worst = max(worst, ref.ratio)
        finally:
            h.close()
    print("EXACT-TAIL greedy %s V=%d log-probability error %.3f of LOGP_TOL" % (tag, V, worst))


@pytest.mark.parametrize("handle", [HANDLES[0], HANDLES[3]], ids=_ids([HANDLES[0], HANDLES[3]]))
def test_greedy_tail_on_rows_without_a_number(dev, handle):
    """V = 40 (lanes 40..63 hold no column): every logit +-inf, rows of -inf alone from step 8 on; then every token banned."""
    tag, bf16, B = handle
    p = greedy_probe(40, B, "inf")
    h = Handle(dev, p, bf16)
    try:
        for ban in (None, et.greedy_ban(40)):
            for logp in (False, True):
                check_greedy_run("greedy inf %s ban=%d logp=%d" % (tag, ban is not None, logp), p, bf16, h.greedy(ban, logp), ban, logp)
    finally:
        h.close()
    for V in (40, 65):
        p = greedy_probe(V, B, "open")
        h = Handle(dev, p, bf16)
        try:
            ban = np.ones(V, dtype=bool)
            for logp in (False, True):
                ref = check_greedy_run("greedy all banned %s V=%d logp=%d" % (tag, V, logp), p, bf16, h.greedy(ban, logp), ban, logp)
                assert bool((ref.tokens == 0).all()) and bool(torch.isnan(ref.logp).all())
        finally:
            h.close()


def test_greedy_state_of_256_rows(dev):
    """32 workgroups fold the finished flags: the exact step at which the last of 256 rows emits EOS (closed), and ST_ALL = 0,
    fin = -1 while one row never does (open).  Unbanned, no log-probabilities."""
    tag, bf16, B = BIG
    for variant in ("open", "closed"):
        p = greedy_probe(1536, B, variant)
        h = Handle(dev, p, bf16)
        try:
            ref = check_greedy_run("greedy %s %s" % (tag, variant), p, bf16, h.greedy(), None, False)
        finally:
            h.close()
        led = et.greedy_ledger(p, ref)
        assert {"fin:same-wg", "fin:diff-wg"} <= led and ("fin:never" if variant == "open" else "fin:early") in led


# ---- b. the sampled tail: dec_sample<BAN, LOGP>, the wrapper ------------------------------------------------------------------------

@pytest.mark.parametrize("case", et.SAMPLED, ids=[c[0] for c in et.SAMPLED])
def test_sampled_tail_draws_with_the_counter_of_row_and_step(dev, case):
    """Row b at step t takes sample_ref's token for u = uniform(seed, b, t); finished rows emit pad; rows without a
    distribution take the greedy token; the log-probability is the greedy one; a second seed replays the captured step."""
    tag, V, B, bf16, use_ban, top_k, seeds = case
    p = greedy_probe(V, B, "open")
    ban = et.greedy_ban(V) if use_ban else None
    h = Handle(dev, p, bf16)
    try:
        n, seen = 0, []
        for logp in (False, True):
            n += 1
            for seed in seeds:
                samp = (seed, 1.0, top_k, 1.0)
                got = h.greedy(ban, logp, samp)
                assert got.captures == n, "a new seed must replay the captured step"
                ref = check_greedy_run("sampled %s seed %d logp=%d" % (tag, seed, logp), p, bf16, got, ban, logp, samp)
                assert float(ref.edge[np.isfinite(ref.edge)].min()) > et.sr.SLACK    # no draw is decided by the slack
                seen.append(got.tokens)
            assert not torch.equal(seen[-1], seen[-2])
    finally:
        h.close()


# ---- c. beam select, scorer and finalize: dec_beam_select, dec_beam_finalize_kernel ------------------------------------------------

def _beam_case(dev, case):
    tag, k, G, V, T, lp, kind, bf16, seed = case
    p, ban = et.beam_case(case)
    et.check_tail_probe(p)
    h = Handle(dev, p, bf16)
    try:
        got = h.beam(k, G, lp, ban)
    finally:
        h.close()
    copy = None if bf16 else got.logits
    ref = et.beam_trace(p, lp, ban, copy=copy)                                # tests/beam_ref.py on the design (the copy on f32)
    check_logits("beam " + tag, p, bf16, got, ref)
    err = et.check_beam("beam " + tag, got, ref, k)
    emu = et.beam_trace(p, lp, ban, copy=copy, cls=et.BeamEmu)
    gap = et.check_margins("beam " + tag, emu.ref.gaps, err)                  # a designed tie, or clear of 2 x the score error
    sc = np.concatenate([np.stack(ref.scores).ravel()] + [np.array([e[0] for h in hs for e in h]) for hs in ref.hyps])
    live = np.abs(sc[np.isfinite(sc)])
    print("EXACT-TAIL beam %s score error %.3e of tolerance %.3e, smallest untied gap %.3e" % (
        tag, err, float(et.beam_tol(live.max())) if len(live) else 0.0, gap))
    return got, ref, emu


@pytest.mark.parametrize("case", et.BEAM, ids=[c[0] for c in et.BEAM])
def test_beam_search_on_designed_logits(dev, case):
    """After every step: backptr (both fields), tokens_out, beam_scores, the hypothesis records in list order, the poll triple;
    after finalize: out_ids, hyps[g][3], out_logp and its sum (the NaN case too: a NaN score compares false both ways, as
    include/mrmt3_hip.h now says)."""
    _beam_case(dev, case)


def test_beam_search_of_256_rows(dev):
    got, ref, emu = _beam_case(dev, et.BEAM_BIG)
    assert "group:done-while-others-run" in emu.ref.events


def test_beam_lds_limit_is_exact(dev):
    """k = 8, V = 2048 (64 KiB of candidate scores beside the kernel's static arrays) runs: the case above.  One column more is
    refused with MRMT3_ERR_INVALID_ARG: nothing is launched, the caller's buffers keep their contents."""
    p = et.beam_design(2049, 8, 1, 4, 0)
    h = Handle(dev, p, True)
    try:
        h.beam_buffers(1)
        with torch.cuda.stream(h.stream):
            h.tokens.fill_(-9)
            rc = h.begin_beam(8, 1, 1.0, None)
        h.stream.synchronize()
        assert rc == 1, rc                                                     # MRMT3_ERR_INVALID_ARG
        assert bool((h.tokens == -9).all()) and bool((h.bp == -9).all()) and bool((h.hyp == -9).all()) and bool((h.bscore == 123.0).all())
    finally:
        h.close()


# ---- d. the KV-cache reorder: dec_beam_reorder, every slot, both layers ------------------------------------------------------------

def _reorder_case(dev, case):
    tag, k, G, read_layer, bf16, seed = case
    p = et.reorder_probe(k, G, read_layer, seed)
    et.check_reorder_probe(p)
    h = Handle(dev, p, bf16)
    try:
        got = h.beam(k, G, 1.0, p.ban)
    finally:
        h.close()
    ratio, tr = et.check_reorder("reorder " + tag, p, got.logits, bf16, got.bp)   # backpointers, then every read-out element
    err = et.check_beam("reorder " + tag, got, tr, k)
    emu = et.beam_trace(p, 1.0, p.ban, copy=got.logits, design=False, cls=et.BeamEmu)
    gap = et.check_margins("reorder " + tag, emu.ref.gaps, err)
    maps = et.reorder_ledger(p, tr)
    print("EXACT-TAIL reorder %s read-out error %.3f of ATTN_TOL, score error %.3e, smallest gap %.3e, parent maps %s" % (
        tag, ratio, err, gap, sorted(maps)))
    return maps


@pytest.mark.parametrize("case", et.REORDER, ids=[c[0] for c in et.REORDER])
def test_reorder_moves_every_slot_of_both_layers(dev, case):
    """28 steps, 3 groups: the step's logits show (V[fresh] + V[old]) / 2 of the read layer's cache, every element, against the
    holders followed through the reference's backpointers (read1: V unique per row; read0: layer 0, unique per history)."""
    maps = _reorder_case(dev, case)
    assert {"fan-out", "swap"} <= maps and ("all-moved-k8" in maps if case[1] == 8 else {"identity", "3-cycle"} <= maps)


@pytest.mark.parametrize("case", et.REORDER_BIG, ids=[c[0] for c in et.REORDER_BIG])
def test_reorder_of_32_groups(dev, case):
    assert "all-moved-k8" in _reorder_case(dev, case)
