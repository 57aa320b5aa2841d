"""Greedy generation on the MI355X decoder (csrc/decode.hip, decode_tail.hip, decode_grammar.hip) with the reference's output contract.

  * `T5ForConditionalGeneration.generate` (models/t5.py:251-302): batched; returns int64
    [B, 1 + steps] starting with token 0, finished rows padded with 0, stops when every row has
    emitted EOS.
  * `T5SegMemV2.generate` / `T5SegMemV2WithPrev.generate` (t5_segmem_v2.py:169-233,
    t5_segmem_v2_with_prev.py:226-296): segments decoded one after the other, each conditioned on
    the previous segment's tokens through the segment-memory encoder; returns [n_seg, max_length].
The encoder, the segment-memory encoder and the cross-attention K/V projections run through the
same engine kernels as training; only the token loop uses the KV-cached step graph.

`generate_beam` adds what the reference's call site asks of HF `generate` (inference.py:186-190) and its custom
`generate` drops: beam search (HF 4.18 `beam_search` + `BeamSearchScorer`, early_stopping=False, one hypothesis
kept; `max_length` counts new tokens as above) and single-token bans (`bad_token_ids`, HF `NoBadWordsLogitsProcessor`).
`num_beams=1` is the greedy decode with the ban, as HF dispatches it.

`return_logprobs=True` (every entry point): `(ids, logp)` instead of `ids`, `logp` f32 of the shape of `ids` with
the log-probability the model gave each emitted token at its position, 0.0 for the start token and for padding.

`do_sample=True` (every entry point but the beam search): the step draws its token from the distribution HF's
`sample()` builds (ban, `temperature`, `top_k`, `top_p`) instead of taking the argmax; the draw is a pure function of
(`seed`, row of the decode batch, token step).  `generate_sample` / `generate_best_of` draw several transcriptions per segment.

`constrained=True` (every entry point): only token sequences the MT3 event decoder accepts.  The event grammar is a
state machine per decode row on the device, advanced inside the captured step; its per-row mask acts where `bad_token_ids`
acts.  Along a memory chain (`_decode_chains`, `generate_2`) segment i + 1 starts from the notes segment i left sounding.

Structure: every entry point folds its keywords into one `_Options` record.  `Decoder.decode` decodes one batch in any mode
(greedy, sampled, n samples per segment, beam) and returns owned `(ids, logp)`.  Three loops call it: `_decode_batched`
(plain T5 and `segmem_v1`: chunks of `MAX_DECODE_BATCH` rows, padded and stacked), `_decode_chains` (the segment-memory
chain of S recordings in lockstep; `generate` / `generate_beam` are S = 1, `generate_songs` groups of S) and `generate_2`'s
prefix chain (the memory is a decoder prefix there, not extra cross-attention rows).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, replace

import torch

from . import lib
from .grammar import ACTIVE_BYTES, EventGrammar, resolve as _grammar


MAX_DECODE_BATCH = 256     # DEC_MAXB of csrc/decode.h: sequences decoded together (one wave per row x sequence)
MAX_BEAMS = 8              # BEAM_MAXK of csrc/decode_tail.hip
BEAM_HREC = 32             # int32 per group of the hypothesis record (csrc/decode_tail.hip, include/mrmt3_hip.h)


MAX_SAMPLE_VOCAB = 2048   # 64 * LOGP_REGS of csrc/decode.h: the sampled tail keeps a vocabulary row in one wave's registers


@dataclass(frozen=True)
class Sampling:
    """What `mrmt3_decoder_set_sampling` takes: `temperature` > 0, `top_k` (0 = off), `top_p` in (0, 1] (1 = off), `seed`."""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0

    def __post_init__(self):
        t, p = self.temperature, self.top_p
        if not (isinstance(t, (int, float)) and math.isfinite(t) and t > 0):
            raise ValueError(f"temperature must be a finite number > 0, got {t!r}")
        if not (isinstance(self.top_k, int) and self.top_k >= 0):
            raise ValueError(f"top_k must be an int >= 0 (0 = off), got {self.top_k!r}")
        if not (isinstance(p, (int, float)) and 0.0 < p <= 1.0):
            raise ValueError(f"top_p must lie in (0, 1], got {p!r}")
        if not (isinstance(self.seed, int) and 0 <= self.seed < 2 ** 64):
            raise ValueError(f"seed must be an int in [0, 2^64), got {self.seed!r}")

    def shifted(self, i: int) -> "Sampling":
        """The same parameters with `seed + i`: decodes that reuse row counters (the next batch, the next segment of a
        memory chain) must not share draws."""
        return replace(self, seed=(self.seed + i) % 2 ** 64)


def _sampling(do_sample, temperature, top_k, top_p, seed):
    """The sampling keywords of the entry points -> `Sampling`, or None for `do_sample=False` (then nothing is looked at)."""
    return Sampling(temperature, top_k, top_p, seed) if do_sample else None


@dataclass(frozen=True)
class _Options:
    """What an entry point's keywords say about the decode, built once per call and handed down the loops."""
    num_beams: int = 1
    length_penalty: float = 1.0
    bad_token_ids: object = None
    sampling: "Sampling | None" = None
    return_logprobs: bool = False
    poll_every: int = 64
    n: int = 1                     # rows per segment of a sampled decode (`num_return_sequences`)
    through_poll: bool = False     # greedy / sampled ids run to the last step replayed, not to the finish step (`generate_songs`)
    grammar: "EventGrammar | None" = None   # constrained decoding (`constrained=`): the event grammar every row obeys

    @property
    def rows(self) -> int:
        """Decode-batch rows per segment."""
        return self.num_beams * self.n


class _Weights(C.Structure):
    _fields_ = [("embed", C.c_void_p), ("pos", C.c_void_p), ("lm_head", C.c_void_p), ("final_ln", C.c_void_p)] + \
               [(n, C.POINTER(C.c_void_p)) for n in ("ln_self", "w_qkv", "w_o_self", "ln_cross", "w_q_cross",
                                                     "w_o_cross", "ln_ff", "w_wi", "w_wo")]


class Decoder:
    """Owns one mrmt3_decoder handle (KV cache, scratch, captured graph) for a model."""

    def __init__(self, model, max_batch: int, max_len: int, max_enc_len: int):
        self.model = model
        eng, cfg = model.engine, model.cfg
        self.max_batch, self.max_len, self.max_enc = max_batch, max_len, max_enc_len
        self.dt = eng.dt
        h = C.c_void_p()
        lib._check(lib.load().mrmt3_decoder_create(C.byref(h), cfg["num_decoder_layers"], cfg["d_model"],
                                                   cfg["num_heads"], cfg["d_ff"], cfg["vocab_size"], max_batch,
                                                   max_len, max_enc_len, lib.BF16 if self.dt == torch.bfloat16 else lib.F32,
                                                   cfg["layer_norm_epsilon"]), "decoder_create")
        self.h = h
        self.tokens = torch.zeros(max_batch, max_len + 1, dtype=torch.int64, device=model.device)
        self.pinned = torch.zeros(3, dtype=torch.int32).pin_memory()
        self._wkeep = None
        # hipGraph capture is illegal on the legacy default stream: the token loop runs on its own stream
        self.stream = torch.cuda.Stream(device=model.device)
        # persistent cross-attention K|V buffer: a stable address lets the captured graph be reused
        self.ckv_buf = torch.empty(cfg["num_decoder_layers"] * max_batch * max_enc_len * 2 * eng.inner,
                                   device=model.device, dtype=self.dt)
        # made on first use, then never reallocated: a captured step graph bakes their addresses in
        self._ban_buf = self.logp = self._beam_logp = self._prefix_buf = None
        self._bp = self._bscore = self._hyp = self._beam_out = None

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib.load().mrmt3_decoder_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _weights(self):
        m, eng, f = self.model, self.model.engine, self.model.flat
        L = m.cfg["num_decoder_layers"]

        def arr(fn):
            a = (C.c_void_p * L)(*[fn(i).data_ptr() for i in range(L)])
            return a

        b = lambda i: f"decoder.block.{i}.layer"
        keep = dict(
            ln_self=arr(lambda i: f.master(f"{b(i)}.0.layer_norm.weight")),
            w_qkv=arr(lambda i: eng.W(f"decoder.{i}.qkv")),
            w_o_self=arr(lambda i: eng.W(f"decoder.{i}.o")),
            ln_cross=arr(lambda i: f.master(f"{b(i)}.1.layer_norm.weight")),
            w_q_cross=arr(lambda i: eng.W(f"decoder.{i}.cq")),
            w_o_cross=arr(lambda i: eng.W(f"decoder.{i}.co")),
            ln_ff=arr(lambda i: f.master(f"{b(i)}.2.layer_norm.weight")),
            w_wi=arr(lambda i: eng.W(f"decoder.{i}.wi")),
            w_wo=arr(lambda i: eng.W(f"decoder.{i}.wo")),
        )
        w = _Weights()
        w.embed = f.master("decoder_embed_tokens.weight").data_ptr()
        w.pos = eng.pos(m.device).data_ptr()
        w.lm_head = eng.W("lm_head").data_ptr()
        w.final_ln = f.master("decoder.final_layer_norm.weight").data_ptr()
        for k, a in keep.items():
            setattr(w, k, C.cast(a, C.POINTER(C.c_void_p)))
        self._wkeep = (keep, w)
        return w

    def cross_kv(self, enc_cat, B, Lc):
        """[layers][B*Lc][2*inner] K|V projections of the (memory-augmented) encoder states."""
        eng = self.model.engine
        L = self.model.cfg["num_decoder_layers"]
        out = self.ckv_buf[:L * B * Lc * 2 * eng.inner].view(L, B * Lc, 2 * eng.inner)
        for i in range(L):
            lib.gemm_nt(enc_cat, eng.W(f"decoder.{i}.ckv"), out=out[i])
        return out

    def ban_mask(self, bad_token_ids):
        """Device [V] uint8 mask of `bad_token_ids` in a buffer of stable address (the step graph bakes the pointer in),
        or None when there is nothing to ban."""
        ids = sorted({int(i) for i in (bad_token_ids or ())})
        if not ids:
            return None
        V = self.model.cfg["vocab_size"]
        if ids[0] < 0 or ids[-1] >= V:
            raise ValueError(f"bad_token_ids must lie in [0, {V})")
        if self._ban_buf is None:
            self._ban_buf = torch.zeros(V, dtype=torch.uint8, device=self.model.device)
        m = torch.zeros(V, dtype=torch.uint8)
        m[ids] = 1
        self._ban_buf.copy_(m)
        return self._ban_buf

    def cross_kv_beam(self, enc_cat, G, k, Lc):
        """cross_kv of G segments with every segment's rows repeated k times (one per beam): [layers][G*k*Lc][2*inner].
        The projections run once per segment; the step kernels then see k independent rows per group."""
        eng = self.model.engine
        L = self.model.cfg["num_decoder_layers"]
        one = torch.empty(L, G * Lc, 2 * eng.inner, device=enc_cat.device, dtype=self.dt)
        for i in range(L):
            lib.gemm_nt(enc_cat, eng.W(f"decoder.{i}.ckv"), out=one[i])
        out = self.ckv_buf[:L * G * k * Lc * 2 * eng.inner].view(L, G, k, Lc, 2 * eng.inner)
        out.copy_(one.view(L, G, 1, Lc, 2 * eng.inner).expand(L, G, k, Lc, 2 * eng.inner))
        return out.view(L, G * k * Lc, 2 * eng.inner)

    def logp_buffer(self):
        """[max_batch, max_len + 1] f32 beside `tokens`, allocated once (the step graph bakes its address in)."""
        if self.logp is None:
            self.logp = self._f32_rows()
        return self.logp

    def _f32_rows(self):
        return torch.zeros(self.max_batch, self.max_len + 1, dtype=torch.float32, device=self.model.device)

    def prefix_buffer(self, n_pre):
        """[1, n_pre, d] f32 for `generate_2`'s memory rows: one address across segments keeps the captured graph valid."""
        if self._prefix_buf is None or self._prefix_buf.shape[1] != n_pre:
            self._prefix_buf = torch.empty(1, n_pre, self.model.cfg["d_model"], device=self.model.device, dtype=torch.float32)
        return self._prefix_buf

    def _on_stream(self, fn):
        """`fn()` on the decoder's stream, ordered after the caller's work and before what the caller does next."""
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            out = fn()
        cur.wait_stream(self.stream)
        return out

    def _check_logits_out(self, logits_out, steps, B):
        if logits_out is None:
            return
        assert logits_out.dtype == torch.float32 and logits_out.is_contiguous() and logits_out.is_cuda
        assert logits_out.dim() == 3 and logits_out.shape[0] >= steps and \
            tuple(logits_out.shape[1:]) == (B, self.model.cfg["vocab_size"]), tuple(logits_out.shape)

    def decode(self, enc_rows, G, Lc, max_steps, o: _Options, shift=0, prefix=None, carry=None):
        """One decode batch in the mode `o` names: G segments' encoder rows [G * Lc, d], `o.rows` decode rows per segment
        (beam j / sample j of segment g is row g * o.rows + j), sampled with `seed + shift`.  -> (ids [rows, W] int64, logp
        [rows, W] f32 or None), owned: the start token first, nothing stale.  Greedy / sampled: rows = G * o.n and W = 1 +
        the step the last row finished at (`max_steps` when one never did; with `o.through_poll` 1 + the token steps
        replayed, finished rows padded to there).  Beam: rows = G and W is `run_beam`'s.
        With `o.grammar` the decode is constrained; `carry` [G, 2048] uint8 (or None) holds the notes sounding when each
        segment began (`grammar_active` afterwards: the notes each returned row leaves sounding)."""
        if o.grammar is not None:
            o.grammar.check_ban(o.bad_token_ids)
            if carry is not None and o.rows > 1:
                carry = carry.repeat_interleave(o.rows, 0)
        if o.num_beams > 1:
            ckv = self.cross_kv_beam(enc_rows, G, o.num_beams, Lc)
            ids, _, _, *lp = self.run_beam(ckv, G, o.num_beams, Lc, max_steps, o.length_penalty, self.ban_mask(o.bad_token_ids),
                                           o.poll_every, return_logprobs=o.return_logprobs, grammar=o.grammar, carry=carry)
            return ids.clone(), lp[0].clone() if lp else None
        ckv = self.cross_kv(enc_rows, G, Lc) if o.n == 1 else self.cross_kv_beam(enc_rows, G, o.n, Lc)
        toks, done, fin, *lp = self.run(ckv, G * o.n, Lc, max_steps, o.poll_every, prefix=prefix,
                                        ban=self.ban_mask(o.bad_token_ids), return_logprobs=o.return_logprobs,
                                        sampling=o.sampling.shifted(shift) if o.sampling else None, grammar=o.grammar,
                                        carry=carry)
        if o.through_poll:
            W = 1 + done - (0 if prefix is None else prefix.shape[1])
        else:
            W = 1 + (fin + 1 if fin >= 0 else max_steps)
        return toks[:G * o.n, :W].clone(), lp[0][:G * o.n, :W].clone() if lp else None

    def run(self, ckv, B, Lc, max_steps, poll_every=64, prefix=None, logits_out=None, ban=None, return_logprobs=False,
            sampling=None, grammar=None, carry=None):
        """Decode up to max_steps tokens for B rows; returns (tokens [B, max_len+1] view, steps run,
        finish_step or -1) and, with `return_logprobs`, a fourth item: the [B, max_len+1] f32 view of each emitted
        token's log-probability (mrmt3_decoder_set_logprobs; the step graph with that tail is captured on first use).  `prefix` [B, n, d] f32: memory rows fed as decoder positions 0..n-1.
        `logits_out` [>= n + max_steps, B, V] f32 device tensor (tests): row s receives step s's lm_head
        output, prefix steps included; steps are then replayed one at a time, each followed by a copy.
        `ban`: device [V] uint8 mask (`ban_mask`) of tokens the argmax never picks, or None.
        `sampling`: a `Sampling` (or a (temperature, top_k, top_p, seed) tuple): row b draws its token of step t with the
        counter (b, t) (mrmt3_decoder_set_sampling; the sampled step is captured once, a new seed or parameters replay it).
        `grammar`: an `EventGrammar`: every row obeys it (mrmt3_decoder_set_grammar), `ban` OR-ed into its masks; `carry`
        [B, 2048] uint8 device bit sets of the notes sounding when each row's segment began, or None."""
        if sampling is not None and not isinstance(sampling, Sampling):
            sampling = Sampling(*sampling)
        if sampling is not None and self.model.cfg["vocab_size"] > MAX_SAMPLE_VOCAB:
            raise ValueError(f"sampling needs vocab_size <= {MAX_SAMPLE_VOCAB}")
        self._sampling = sampling
        self._ban = ban
        self._set_grammar_args(grammar, carry, B)
        self._logp = self.logp_buffer() if return_logprobs else None
        cfg = self.model.cfg
        l = lib.load()
        w = self._weights()
        self._ckv = ckv
        self._check_logits_out(logits_out, (0 if prefix is None else prefix.shape[1]) + max_steps, B)
        out = self._on_stream(lambda: self._run_on_stream(l, w, ckv, B, Lc, max_steps, poll_every, cfg, prefix, logits_out))
        return out + (self._logp,) if return_logprobs else out

    def _run_on_stream(self, l, w, ckv, B, Lc, max_steps, poll_every, cfg, prefix=None, logits_out=None):
        lib._check(l.mrmt3_decoder_begin(self.h, C.byref(w), lib._p(ckv), B, Lc, lib._p(self.tokens),
                                         cfg["decoder_start_token_id"], cfg["eos_token_id"], cfg["pad_token_id"],
                                         lib._stream()), "decoder_begin")
        if self._ban is not None:
            lib._check(l.mrmt3_decoder_set_ban(self.h, lib._p(self._ban), lib._stream()), "decoder_set_ban")
        if self._logp is not None:
            lib._check(l.mrmt3_decoder_set_logprobs(self.h, lib._p(self._logp), self._logp.stride(0), lib._stream()),
                       "decoder_set_logprobs")
        if self._sampling is not None:
            sp = self._sampling
            lib._check(l.mrmt3_decoder_set_sampling(self.h, float(sp.temperature), int(sp.top_k), float(sp.top_p),
                                                    int(sp.seed), lib._stream()), "decoder_set_sampling")
        self._set_grammar(l)
        if prefix is not None:
            n_pre = prefix.shape[1]
            assert prefix.dtype == torch.float32 and prefix.is_contiguous() and prefix.shape[0] == B
            assert n_pre + max_steps <= self.max_len, "prefix + token steps exceed the decoder's max_len"
            self._prefix = prefix        # keep alive while the graph may read it
            lib._check(l.mrmt3_decoder_set_prefix(self.h, lib._p(prefix), n_pre, lib._stream()), "decoder_set_prefix")
            max_steps += n_pre
        done, fin = self._loop(l, B, max_steps, poll_every, logits_out)
        return self.tokens, done, fin

    def _set_grammar_args(self, grammar, carry, rows):
        if carry is not None:
            assert grammar is not None and carry.dtype == torch.uint8 and carry.is_cuda and carry.is_contiguous() and \
                tuple(carry.shape) == (rows, ACTIVE_BYTES), "carry: [rows, 2048] uint8 on the device"
        self._gram = (grammar.c_struct(), carry) if grammar is not None else None     # kept alive through the decode

    def _set_grammar(self, l):
        """After begin / begin_beam and the ban: the start states and the step-0 masks, on the current stream."""
        if self._gram is not None:
            g, carry = self._gram
            lib._check(l.mrmt3_decoder_set_grammar(self.h, C.byref(g), lib._p(carry), lib._stream()), "decoder_set_grammar")

    def grammar_active(self, rows):
        """[rows, 2048] uint8, owned: the `active` set each row of the last constrained decode ends with (beam: each group's
        returned hypothesis), mrmt3_decoder_grammar_active."""
        out = torch.empty(rows, ACTIVE_BYTES, dtype=torch.uint8, device=self.model.device)
        self._on_stream(lambda: lib._check(lib.load().mrmt3_decoder_grammar_active(self.h, lib._p(out), lib._stream()),
                                           "decoder_grammar_active"))
        return out

    def _loop(self, l, B, max_steps, poll_every, logits_out):
        """Replay steps until max_steps or every row (greedy) / group (beam) is done; (steps run, finish step or -1)."""
        done, fin = 0, -1
        while done < max_steps:
            n = min(poll_every, max_steps - done)
            if logits_out is None:
                lib._check(l.mrmt3_decoder_run(self.h, n, lib._stream()), "decoder_run")
            else:
                for i in range(n):
                    lib._check(l.mrmt3_decoder_run(self.h, 1, lib._stream()), "decoder_run")
                    lib._check(l.mrmt3_decoder_logits(self.h, lib._p(logits_out[done + i]), B, lib._stream()),
                               "decoder_logits")
            done += n
            lib._check(l.mrmt3_decoder_poll(self.h, C.c_void_p(self.pinned.data_ptr()), lib._stream()), "decoder_poll")
            torch.cuda.current_stream().synchronize()
            if int(self.pinned[1]):
                fin = int(self.pinned[2])
                break
        return done, fin

    def run_beam(self, ckv, G, k, Lc, max_steps, length_penalty=1.0, ban=None, poll_every=64, logits_out=None,
                 return_logprobs=False, grammar=None, carry=None):
        """Beam search over G groups of k rows (`cross_kv_beam`).  Returns (ids [G, W] int64, steps run, finish step or
        -1): start token, the best hypothesis, EOS when shorter than 1 + max_steps, pad; W = min(longest + 1,
        1 + max_steps).  `logits_out` [>= max_steps, G*k, V] f32 (tests) as in `run`.  After the call `bp` [max_len,
        G*k, 2] (parent row, token per step), `beam_scores` [G*k] and `hyps` [G, BEAM_HREC] hold the search state.
        `return_logprobs`: a fourth item, [G, W] f32, the best hypothesis' per-token log-probabilities (the closing EOS
        included; their sum is the hypothesis' raw score).  `grammar`, `carry` [G * k, 2048] as in `run`."""
        B = G * k
        if not (1 <= k <= MAX_BEAMS) or B > self.max_batch or max_steps > self.max_len or max_steps < 1:
            raise ValueError(f"run_beam: need 1 <= k <= {MAX_BEAMS}, G*k <= {self.max_batch}, 1 <= steps <= {self.max_len}")
        self._check_logits_out(logits_out, max_steps, B)
        self._ban, self._ckv = ban, ckv
        self._set_grammar_args(grammar, carry, B)
        l = lib.load()

        def search():
            self.begin_beam(ckv, G, k, Lc, length_penalty, ban)
            self._set_grammar(l)
            done, fin = self._loop(l, B, max_steps, poll_every, logits_out)
            if return_logprobs:
                if self._beam_logp is None:
                    self._beam_logp = self._f32_rows()
                lib._check(l.mrmt3_decoder_beam_finalize_logprobs(self.h, lib._p(self._beam_out), lib._p(self._beam_logp),
                                                                  self.max_len + 1, max_steps, lib._stream()),
                           "decoder_beam_finalize_logprobs")
            else:
                lib._check(l.mrmt3_decoder_beam_finalize(self.h, lib._p(self._beam_out), self.max_len + 1, max_steps,
                                                         lib._stream()), "decoder_beam_finalize")
            return done, fin, self.hyps(G)[:, 3].cpu()             # once per decode

        done, fin, lens = self._on_stream(search)
        W = min(int(lens.max()) + 1, 1 + max_steps)
        if return_logprobs:
            return self._beam_out[:G, :W], done, fin, self._beam_logp[:G, :W]
        return self._beam_out[:G, :W], done, fin

    def begin_beam(self, ckv, G, k, Lc, length_penalty=1.0, ban=None):
        """mrmt3_decoder_begin_beam on the current stream with this decoder's beam buffers (allocated once: the step
        graph bakes their addresses in).  `run_beam` is the whole decode; this is its first step, for tools."""
        cfg = self.model.cfg
        if self._bp is None:
            dev = self.model.device
            self._bp = torch.zeros(self.max_len * self.max_batch * 2, dtype=torch.int32, device=dev)
            self._bscore = torch.zeros(self.max_batch, dtype=torch.float32, device=dev)
            self._hyp = torch.zeros(self.max_batch * BEAM_HREC, dtype=torch.int32, device=dev)
            self._beam_out = torch.zeros(self.max_batch, self.max_len + 1, dtype=torch.int64, device=dev)
        self._ban, self._ckv = ban, ckv
        w = self._weights()
        lib._check(lib.load().mrmt3_decoder_begin_beam(
            self.h, C.byref(w), lib._p(ckv), G, k, Lc, lib._p(self.tokens), cfg["decoder_start_token_id"],
            cfg["eos_token_id"], cfg["pad_token_id"], float(length_penalty), lib._p(ban), lib._p(self._bp),
            lib._p(self._bscore), lib._p(self._hyp), lib._stream()), "decoder_begin_beam")

    def backptr(self, rows):
        """[max_len, rows, 2] int32 (parent row, token) of the last beam decode."""
        return self._bp[:self.max_len * rows * 2].view(self.max_len, rows, 2)

    def beam_scores(self, rows):
        return self._bscore[:rows]

    def hyps(self, G):
        return self._hyp[:G * BEAM_HREC].view(G, BEAM_HREC)

    @property
    def graph_captured(self) -> bool:
        return bool(lib.load().mrmt3_decoder_graph_captured(self.h))

    @property
    def capture_count(self) -> int:
        """Step graphs captured by this handle so far (a replay of the captured step adds none)."""
        return int(lib.load().mrmt3_decoder_capture_count(self.h))


def _decoder_for(model, B, max_len, enc_len) -> Decoder:
    dec = getattr(model, "_decoder", None)
    if dec is None or dec.max_batch < B or dec.max_len < max_len or dec.max_enc < enc_len or \
            dec.dt != model.engine.dt or dec.tokens.device != model.device:
        dec = Decoder(model, max(B, 1), max_len, enc_len)
        model._decoder = dec
    return dec


@torch.no_grad()
def generate(model, inputs, max_length=1024, poll_every=64, return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0,
             constrained=False):
    return _generate(model, inputs, max_length, _Options(sampling=_sampling(do_sample, temperature, top_k, top_p, seed),
                                                         return_logprobs=return_logprobs, poll_every=poll_every,
                                                         grammar=_grammar(constrained, model)))


@torch.no_grad()
def generate_sample(model, inputs, max_length=1024, temperature=1.0, top_k=0, top_p=1.0, seed=0, num_return_sequences=1,
                    bad_token_ids=None, return_logprobs=False, poll_every=64, constrained=False):
    """`generate` that draws.  Plain T5: `num_return_sequences = n` transcriptions per segment, row g * n + j of the
    [B * n, W] output is sample j of segment g (its cross K|V repeated as the beam search's are; the row's draw counter is
    its row in the decode batch).  Segment-memory models decode one sample per segment along their memory chain."""
    return _generate(model, inputs, max_length, _Options(bad_token_ids=bad_token_ids,
                                                         sampling=Sampling(temperature, top_k, top_p, seed),
                                                         return_logprobs=return_logprobs, poll_every=poll_every,
                                                         n=num_return_sequences, grammar=_grammar(constrained, model)))


def best_of_select(ids, logp, n, eos_token_id):
    """Of every n consecutive rows of `ids` / `logp` [G * n, W], the one whose log-probabilities, summed over the emitted
    tokens up to and including the first EOS (the whole row when there is none), are highest; ties go to the lowest j.
    -> (ids [G, W], logp [G, W], j [G]).  Torch ops on the tensors' device, no loop over rows."""
    if ids.shape != logp.shape or ids.shape[0] % n:
        raise ValueError(f"best_of_select: ids {tuple(ids.shape)} / logp {tuple(logp.shape)} are not G * {n} matching rows")
    is_eos = (ids[:, 1:] == eos_token_id).long()
    live = (torch.cumsum(is_eos, -1) - is_eos) == 0                  # up to and including the first EOS
    score = torch.where(live, logp[:, 1:].double(), torch.zeros((), dtype=torch.float64, device=logp.device)).sum(-1)
    j = torch.argmax(score.view(-1, n), dim=1)                       # the first of equal maxima
    rows = torch.arange(j.shape[0], device=ids.device) * n + j
    return ids[rows], logp[rows], j


@torch.no_grad()
def generate_best_of(model, inputs, n, max_length=1024, temperature=1.0, top_k=0, top_p=1.0, seed=0, bad_token_ids=None,
                     poll_every=64, constrained=False):
    """n samples per segment (`generate_sample`), the most likely one kept: (ids [B, W], logp [B, W]).  Plain T5 only."""
    if not (isinstance(n, int) and n >= 1):
        raise ValueError(f"n must be an int >= 1, got {n!r}")
    if model.VARIANT not in ("t5", "segmem_v1"):
        raise ValueError("generate_best_of is for the plain T5 decode; the segment-memory chain decodes one sample per segment")
    ids, logp = generate_sample(model, inputs, max_length, temperature, top_k, top_p, seed, n, bad_token_ids, True, poll_every,
                                constrained)
    ids, logp, _ = best_of_select(ids, logp, n, model.cfg["eos_token_id"])
    return ids, logp


def _pair(ids, logp, return_logprobs):
    return (ids, logp) if return_logprobs else ids


def _check_beams(num_beams):
    if not (isinstance(num_beams, int) and 1 <= num_beams <= MAX_BEAMS):
        raise ValueError(f"num_beams must be an int in 1..{MAX_BEAMS}, got {num_beams!r}")


def _memory_rows(x, max_length):
    """Ids or log-probabilities [n, W] -> [n, max_length]: cut or zero-padded, as the reference's chain does (`F.pad` / slice)."""
    rows = torch.zeros(x.shape[0], max_length, dtype=x.dtype, device=x.device)
    n = min(x.shape[1], max_length)
    rows[:, :n] = x[:, :n]
    return rows


def _first_memory_ids(max_length, device, with_prev=False):
    """[max_length] memory ids of a recording's first segment; `with_prev`: the V2WithPrev model's."""
    ids = torch.zeros(max_length, dtype=torch.int64, device=device)
    if with_prev:
        ids[0], ids[1] = 1134, 1                         # tie token + EOS (t5_segmem_v2_with_prev.py:257-258)
    else:
        ids[0] = 1                                       # t5_segmem_v2.py:199, t5_segmem.py:190-196
    return ids


def _memory(eng, seg_ids, B, L, Ls):
    """Memory vectors of the previous segment; `segmem_length=0` (the reference's no-memory ablation,
    `[:, :0]`) yields an empty block without touching the memory encoder."""
    if Ls == 0:
        return torch.empty(B, 0, eng.d, device=seg_ids.device, dtype=eng.dt)
    return eng.segmem(seg_ids, B, L)


def _stack(parts, pad_token_id):
    """Decode batches' (ids, logp) -> one: the reference stops when ALL rows are finished, so the narrower batches are
    padded to the widest, ids with `pad_token_id` and log-probabilities with 0.0."""
    if len(parts) == 1:
        return parts[0]
    W = max(ids.shape[1] for ids, _ in parts)
    wide = lambda x, fill: torch.cat([x, x.new_full((x.shape[0], W - x.shape[1]), fill)], 1)
    return (torch.cat([wide(ids, pad_token_id) for ids, _ in parts]),
            torch.cat([wide(lp, 0.0) for _, lp in parts]) if parts[0][1] is not None else None)


def _decode_batched(model, enc, B, Le, max_length, o):
    """Plain T5 (and T5SegMem.generate, which ignores the memory: t5_segmem.py:254-311): the B segments in decode batches
    of MAX_DECODE_BATCH rows, batch c sampled with `seed + c`.  -> (ids [B * o.rows / num_beams, W], logp or None)."""
    per = MAX_DECODE_BATCH // o.rows
    parts = []
    for c, b0 in enumerate(range(0, B, per)):
        G = min(per, B - b0)
        dec = _decoder_for(model, G * o.rows, max_length, Le)
        parts.append(dec.decode(enc.view(B, Le, -1)[b0:b0 + G].reshape(G * Le, -1), G, Le, max_length, o, shift=c))
    return _stack(parts, model.cfg["pad_token_id"])


def _decode_chains(model, songs, max_length, o):
    """The segment-memory chain (V2 / V2WithPrev) of S recordings in lockstep: row s of decode batch i is recording s's
    segment i, its encoder states followed by the memory encoder's view of that recording's segment i - 1 as decoded, cut
    or zero-padded to max_length; segment i is sampled with `seed + i`.  A recording shorter than the longest drops out.
    `songs`: list of [n_seg_s, Le, d].  -> (list of ids [n_seg_s, max_length], list of their logp or []).
    Constrained (`o.grammar`): segment i + 1 of a recording starts with `carry` = the notes segment i left sounding: the
    `active` set of its row as returned, i.e. cut to max_length (`lib.grammar_replay`, device to device).  A recording's
    first segment starts from the empty set: nothing sounds before a recording begins, so its tie section can declare nothing."""
    eng = model.engine
    S, dev = len(songs), songs[0].device
    Le, d = songs[0].shape[1], songs[0].shape[2]
    Ls = min(model.segmem_length, max_length)            # `[:, :segmem_length]` of a max_length-long sequence
    enc = [eng.encode(x).view(x.shape[0], Le, d) for x in songs]           # per recording, all its segments
    prev = [_first_memory_ids(max_length, dev, model.VARIANT == "segmem_v2_with_prev")] * S
    outs = [[] for _ in range(S)]
    outs_lp = [[] for _ in range(S)]
    sounding = [None] * S
    for i in range(max(x.shape[0] for x in songs)):
        live = [s for s in range(S) if i < songs[s].shape[0]]
        B = len(live)
        mem = _memory(eng, torch.stack([prev[s] for s in live]), B, max_length, Ls)       # [B, Ls, d]
        cur = torch.cat([torch.stack([enc[s][i] for s in live]), mem.to(enc[0].dtype)], 1).contiguous()
        dec = _decoder_for(model, B * o.rows, max_length, Le + Ls)
        carry = None
        if o.grammar is not None:
            carry = torch.stack([sounding[s] for s in live]) if i > 0 else torch.zeros(B, ACTIVE_BYTES, dtype=torch.uint8, device=dev)
        ids, lp = dec.decode(cur.view(B * (Le + Ls), d), B, Le + Ls, max_length, o, shift=i, carry=carry)
        rows = _memory_rows(ids, max_length)
        rows_lp = _memory_rows(lp, max_length) if lp is not None else None
        left = lib.grammar_replay(o.grammar, rows, model.cfg["vocab_size"], carry) if o.grammar is not None else None
        for r, s in enumerate(live):
            outs[s].append(rows[r])
            if lp is not None:
                outs_lp[s].append(rows_lp[r])
            prev[s] = rows[r]
            if left is not None:
                sounding[s] = left[r]
    return [torch.stack(x) for x in outs], [torch.stack(x) for x in outs_lp if x]


def _generate(model, inputs, max_length, o):
    """`generate`, `generate_sample` and `generate_beam` behind their keyword checks: [B, Le, d] segments of one recording
    -> ids, or (ids, logp) with `o.return_logprobs`."""
    if not (isinstance(o.n, int) and 1 <= o.n <= MAX_DECODE_BATCH):
        raise ValueError(f"num_return_sequences must be an int in 1..{MAX_DECODE_BATCH}, got {o.n!r}")
    if o.n > 1 and (o.sampling is None or model.VARIANT not in ("t5", "segmem_v1")):
        raise ValueError("num_return_sequences > 1 needs sampling and the plain T5 decode: the segment-memory chain "
                         "decodes one sample per segment")
    if not inputs.is_cuda:
        raise RuntimeError("generate needs device tensors (no CPU fallback)")
    model.engine.prepare(False)
    if inputs.dtype not in (torch.float32, torch.bfloat16):
        inputs = inputs.float()
    if model.VARIANT in ("t5", "segmem_v1"):
        B, Le, _ = inputs.shape
        return _pair(*_decode_batched(model, model.engine.encode(inputs), B, Le, max_length, o), o.return_logprobs)
    ids, lp = _decode_chains(model, [inputs], max_length, o)
    return _pair(ids[0], lp[0] if lp else None, o.return_logprobs)


@torch.no_grad()
def generate_2(model, inputs, max_length=1024, poll_every=64, num_beams=1, return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0,
               constrained=False):
    """`T5SegMem.generate_2` (models/t5_segmem.py:172-252): segments one after the other; the previous
    segment's tokens go through the segment-memory encoder and its first `segmem_length` outputs are
    PREPENDED to the decoder's input embeddings.  With the KV cache that is a prefix fill: the memory
    rows are fed as decoder positions 0..Ls-1 (self-attention K/V only), tokens start at position Ls.
    A stable prefix buffer keeps the captured step graph valid across segments.  No beam search here.
    `do_sample`: the token steps draw (segment i with `seed + i`), the prefix steps draw nothing.
    `constrained`: the token steps obey the event grammar (the prefix steps leave its state alone); segment i + 1 starts
    from the notes segment i left sounding, the first from none."""
    if num_beams != 1:
        raise ValueError("generate_2 (memory-prefixed decode) has no beam search")
    o = _Options(sampling=_sampling(do_sample, temperature, top_k, top_p, seed), return_logprobs=return_logprobs,
                 poll_every=poll_every, grammar=_grammar(constrained, model))
    eng = model.engine
    if not inputs.is_cuda:
        raise RuntimeError("generate_2 needs device tensors (no CPU fallback)")
    Ls = model.segmem_length
    assert max_length >= Ls, "the reference asserts segmem_length memory rows (t5_segmem.py:213)"
    eng.prepare(False)
    B, Le, d = inputs.shape
    enc = eng.encode(inputs)
    seg_ids = _first_memory_ids(max_length, inputs.device)[None]
    dec = _decoder_for(model, 1, max_length + Ls, Le)
    pre = dec.prefix_buffer(Ls)
    outs, outs_lp = [], []
    sounding = torch.zeros(1, ACTIVE_BYTES, dtype=torch.uint8, device=inputs.device) if o.grammar is not None else None
    for i in range(B):
        if Ls:
            pre.copy_(eng.segmem(seg_ids, 1, max_length).float().view(1, Ls, d))
        ids, lp = dec.decode(enc.view(B, Le, d)[i].contiguous(), 1, Le, max_length, o, shift=i, prefix=pre if Ls else None,
                             carry=sounding)
        seg_ids = _memory_rows(ids, max_length)
        if o.grammar is not None:
            sounding = lib.grammar_replay(o.grammar, seg_ids, model.cfg["vocab_size"], sounding)
        outs.append(seg_ids)
        if lp is not None:
            outs_lp.append(_memory_rows(lp, max_length))
    return _pair(torch.cat(outs, 0), torch.cat(outs_lp, 0) if outs_lp else None, return_logprobs)


@torch.no_grad()
def generate_songs(model, songs, max_length=1024, poll_every=64, num_beams=1, length_penalty=1.0, bad_token_ids=None,
                   return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, constrained=False):
    """Several recordings decoded in lockstep with the segment-memory models (V2 / V2WithPrev).

    The reference transcribes one recording at a time because segment i needs segment i-1's tokens
    (t5_segmem_v2_with_prev.py:241-294) — but recordings are independent of each other.  Here row s of the
    decode batch is recording s's CURRENT segment: every recording keeps its own memory chain, and each row
    produces exactly what `generate` produces for that recording alone (same kernels, one wave per row and
    sequence).  `songs`: list of [n_seg_s, Le, 512] device tensors.  Returns a list of [n_seg_s, max_length]
    int64 tensors.  `num_beams` > 1: recording s is group s of a beam search (`generate_beam` per recording, in
    lockstep); `bad_token_ids` bans tokens in either mode.  The defaults are the greedy decode above.
    `return_logprobs`: (list of ids, list of [n_seg_s, max_length] f32 log-probabilities), rows cut or zero-padded as the ids.
    `do_sample` (greedy mode only): row s draws segment i with the counter (s, step) under `seed + i`; each recording's
    memory chain carries its sampled tokens."""
    _check_beams(num_beams)
    sampling = _sampling(do_sample, temperature, top_k, top_p, seed)
    if sampling is not None and num_beams > 1:
        raise ValueError("beam search does not sample: do_sample needs num_beams == 1")
    if model.VARIANT not in ("segmem_v2", "segmem_v2_with_prev"):
        raise RuntimeError("generate_songs is for the segment-memory models; plain T5 batches segments directly")
    o = _Options(num_beams, length_penalty, bad_token_ids, sampling, return_logprobs, poll_every, through_poll=True,
                 grammar=_grammar(constrained, model))
    per = MAX_DECODE_BATCH // num_beams
    ids, lp = [], []
    for i in range(0, len(songs), per):
        if songs[i].device.type != "cuda":
            raise RuntimeError("generate_songs needs device tensors (no CPU fallback)")
        model.engine.prepare(False)
        part = _decode_chains(model, songs[i:i + per], max_length, o)
        ids += part[0]
        lp += part[1]
    return _pair(ids, lp, return_logprobs)


@torch.no_grad()
def generate_beam(model, inputs, num_beams=1, max_length=1024, length_penalty=1.0, bad_token_ids=None, poll_every=64,
                  return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, constrained=False):
    """Beam search with optional single-token bans; the output contract of `generate` for the model's variant.

    Plain T5 / T5SegMem: [B, W] int64, W = min(longest best hypothesis + 1, 1 + max_length) over the batch: start
    token, tokens, EOS after a hypothesis shorter than 1 + max_length, pad (HF `BeamSearchScorer.finalize`).  Segment
    memory models: [n_seg, max_length], segments one after the other, each one's memory ids = the previous segment's
    best hypothesis cut or zero-padded to max_length.  `num_beams=1` is the greedy decode (with the ban); without a ban
    it equals `generate` bit for bit.  `do_sample` with `num_beams=1` draws the tokens (`generate`'s keywords); beam
    search does not sample."""
    _check_beams(num_beams)
    sampling = _sampling(do_sample, temperature, top_k, top_p, seed)
    if sampling is not None and num_beams > 1:
        raise ValueError("beam search does not sample: do_sample needs num_beams == 1")
    if not inputs.is_cuda:
        raise RuntimeError("generate_beam needs device tensors (no CPU fallback)")
    return _generate(model, inputs, max_length, _Options(num_beams, length_penalty, bad_token_ids, sampling, return_logprobs,
                                                         poll_every, grammar=_grammar(constrained, model)))
