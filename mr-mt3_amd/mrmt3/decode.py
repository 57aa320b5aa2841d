"""Greedy generation on the MI355X decoder (csrc/decode.hip) with the reference's output contract.

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
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, replace

import torch

from . import lib


MAX_DECODE_BATCH = 256     # DEC_MAXB of csrc/decode.hip: sequences decoded together (one wave per row x sequence)
MAX_BEAMS = 8              # BEAM_MAXK of csrc/decode.hip
BEAM_HREC = 32             # int32 per group of the hypothesis record (csrc/decode.hip, include/mrmt3_hip.h)


MAX_SAMPLE_VOCAB = 2048   # 64 * LOGP_REGS of csrc/decode.hip: the sampled tail keeps a vocabulary row in one wave's registers


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
        if getattr(self, "_ban_buf", None) is None:
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
        if getattr(self, "logp", None) is None:
            self.logp = torch.zeros(self.max_batch, self.max_len + 1, dtype=torch.float32, device=self.model.device)
        return self.logp

    def run(self, ckv, B, Lc, max_steps, poll_every=64, prefix=None, logits_out=None, ban=None, return_logprobs=False,
            sampling=None):
        """Decode up to max_steps tokens for B rows; returns (tokens [B, max_len+1] view, steps run,
        finish_step or -1) and, with `return_logprobs`, a fourth item: the [B, max_len+1] f32 view of each emitted
        token's log-probability (mrmt3_decoder_set_logprobs; the step graph with that tail is captured on first use).  `prefix` [B, n, d] f32: memory rows fed as decoder positions 0..n-1.
        `logits_out` [>= n + max_steps, B, V] f32 device tensor (tests): row s receives step s's lm_head
        output, prefix steps included; steps are then replayed one at a time, each followed by a copy.
        `ban`: device [V] uint8 mask (`ban_mask`) of tokens the argmax never picks, or None.
        `sampling`: a `Sampling` (or a (temperature, top_k, top_p, seed) tuple): row b draws its token of step t with the
        counter (b, t) (mrmt3_decoder_set_sampling; the sampled step is captured once, a new seed or parameters replay it)."""
        if sampling is not None and not isinstance(sampling, Sampling):
            sampling = Sampling(*sampling)
        if sampling is not None and self.model.cfg["vocab_size"] > MAX_SAMPLE_VOCAB:
            raise ValueError(f"sampling needs vocab_size <= {MAX_SAMPLE_VOCAB}")
        self._sampling = sampling
        self._ban = ban
        self._logp = self.logp_buffer() if return_logprobs else None
        cfg = self.model.cfg
        l = lib.load()
        w = self._weights()
        self._ckv = ckv
        if logits_out is not None:
            n_pre = 0 if prefix is None else prefix.shape[1]
            assert logits_out.dtype == torch.float32 and logits_out.is_contiguous() and logits_out.is_cuda
            assert logits_out.dim() == 3 and logits_out.shape[0] >= n_pre + max_steps and \
                tuple(logits_out.shape[1:]) == (B, cfg["vocab_size"]), tuple(logits_out.shape)
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            out = self._run_on_stream(l, w, ckv, B, Lc, max_steps, poll_every, cfg, prefix, logits_out)
        cur.wait_stream(self.stream)
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
        if prefix is not None:
            n_pre = prefix.shape[1]
            assert prefix.dtype == torch.float32 and prefix.is_contiguous() and prefix.shape[0] == B
            assert n_pre + max_steps <= self.max_len, "prefix + token steps exceed the decoder's max_len"
            self._prefix = prefix        # keep alive while the graph may read it
            lib._check(l.mrmt3_decoder_set_prefix(self.h, lib._p(prefix), n_pre, lib._stream()), "decoder_set_prefix")
            max_steps += n_pre
        done, fin = self._loop(l, B, max_steps, poll_every, logits_out)
        return self.tokens, done, fin

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
                 return_logprobs=False):
        """Beam search over G groups of k rows (`cross_kv_beam`).  Returns (ids [G, W] int64, steps run, finish step or
        -1): start token, the best hypothesis, EOS when shorter than 1 + max_steps, pad; W = min(longest + 1,
        1 + max_steps).  `logits_out` [>= max_steps, G*k, V] f32 (tests) as in `run`.  After the call `bp` [max_len,
        G*k, 2] (parent row, token per step), `beam_scores` [G*k] and `hyps` [G, BEAM_HREC] hold the search state.
        `return_logprobs`: a fourth item, [G, W] f32, the best hypothesis' per-token log-probabilities (the closing EOS
        included; their sum is the hypothesis' raw score)."""
        cfg = self.model.cfg
        B = G * k
        if not (1 <= k <= MAX_BEAMS) or B > self.max_batch or max_steps > self.max_len or max_steps < 1:
            raise ValueError(f"run_beam: need 1 <= k <= {MAX_BEAMS}, G*k <= {self.max_batch}, 1 <= steps <= {self.max_len}")
        if logits_out is not None:
            assert logits_out.dtype == torch.float32 and logits_out.is_contiguous() and logits_out.is_cuda
            assert logits_out.dim() == 3 and logits_out.shape[0] >= max_steps and \
                tuple(logits_out.shape[1:]) == (B, cfg["vocab_size"]), tuple(logits_out.shape)
        self._ban, self._ckv = ban, ckv
        l = lib.load()
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self.begin_beam(ckv, G, k, Lc, length_penalty, ban)
            done, fin = self._loop(l, B, max_steps, poll_every, logits_out)
            if return_logprobs:
                if getattr(self, "_beam_logp", None) is None:
                    self._beam_logp = torch.zeros(self.max_batch, self.max_len + 1, dtype=torch.float32,
                                                  device=self.model.device)
                lib._check(l.mrmt3_decoder_beam_finalize_logprobs(self.h, lib._p(self._beam_out), lib._p(self._beam_logp),
                                                                  self.max_len + 1, max_steps, lib._stream()),
                           "decoder_beam_finalize_logprobs")
            else:
                lib._check(l.mrmt3_decoder_beam_finalize(self.h, lib._p(self._beam_out), self.max_len + 1, max_steps,
                                                         lib._stream()), "decoder_beam_finalize")
            lens = self.hyps(G)[:, 3].cpu()             # once per decode
        cur.wait_stream(self.stream)
        W = min(int(lens.max()) + 1, 1 + max_steps)
        if return_logprobs:
            return self._beam_out[:G, :W], done, fin, self._beam_logp[:G, :W]
        return self._beam_out[:G, :W], done, fin

    def begin_beam(self, ckv, G, k, Lc, length_penalty=1.0, ban=None):
        """mrmt3_decoder_begin_beam on the current stream with this decoder's beam buffers (allocated once: the step
        graph bakes their addresses in).  `run_beam` is the whole decode; this is its first step, for tools."""
        cfg = self.model.cfg
        if getattr(self, "_bp", None) is None:
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
def generate(model, inputs, max_length=1024, poll_every=64, return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0):
    return _generate(model, inputs, max_length, poll_every, return_logprobs=return_logprobs,
                     sampling=_sampling(do_sample, temperature, top_k, top_p, seed))


@torch.no_grad()
def generate_sample(model, inputs, max_length=1024, temperature=1.0, top_k=0, top_p=1.0, seed=0, num_return_sequences=1,
                    bad_token_ids=None, return_logprobs=False, poll_every=64):
    """`generate` that draws.  Plain T5: `num_return_sequences = n` transcriptions per segment, row g * n + j of the
    [B * n, W] output is sample j of segment g (its cross K|V repeated as the beam search's are; the row's draw counter is
    its row in the decode batch).  Segment-memory models decode one sample per segment along their memory chain."""
    return _generate(model, inputs, max_length, poll_every, bad_token_ids, return_logprobs,
                     sampling=Sampling(temperature, top_k, top_p, seed), n=num_return_sequences)


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
                     poll_every=64):
    """n samples per segment (`generate_sample`), the most likely one kept: (ids [B, W], logp [B, W]).  Plain T5 only."""
    if not (isinstance(n, int) and n >= 1):
        raise ValueError(f"n must be an int >= 1, got {n!r}")
    if model.VARIANT not in ("t5", "segmem_v1"):
        raise ValueError("generate_best_of is for the plain T5 decode; the segment-memory chain decodes one sample per segment")
    ids, logp = generate_sample(model, inputs, max_length, temperature, top_k, top_p, seed, n, bad_token_ids, True, poll_every)
    ids, logp, _ = best_of_select(ids, logp, n, model.cfg["eos_token_id"])
    return ids, logp


def _pair(ids, logp, return_logprobs):
    return (ids, logp) if return_logprobs else ids


def _generate(model, inputs, max_length, poll_every, bad_token_ids=None, return_logprobs=False, sampling=None, n=1):
    """`return_logprobs`: every tensor of ids has a float twin cut, padded (0.0) and stacked the same way.
    `sampling` (a `Sampling`): the tokens are drawn; decode batch c of a plain T5 and segment i of a memory chain use
    `seed + c` / `seed + i`.  `n` > 1 (plain T5, with `sampling`): n rows per segment, output [B * n, W]."""
    eng, cfg = model.engine, model.cfg
    if not (isinstance(n, int) and 1 <= n <= MAX_DECODE_BATCH):
        raise ValueError(f"num_return_sequences must be an int in 1..{MAX_DECODE_BATCH}, got {n!r}")
    if n > 1 and (sampling is None or model.VARIANT not in ("t5", "segmem_v1")):
        raise ValueError("num_return_sequences > 1 needs sampling and the plain T5 decode: the segment-memory chain "
                         "decodes one sample per segment")
    if not inputs.is_cuda:
        raise RuntimeError("generate needs device tensors (no CPU fallback)")
    eng.prepare(False)
    B, Le, d = inputs.shape
    enc = eng.encode(inputs.float() if inputs.dtype not in (torch.float32, torch.bfloat16) else inputs)
    if model.VARIANT in ("t5", "segmem_v1"):      # T5SegMem.generate ignores the memory (t5_segmem.py:254-311)
        out = []
        per = MAX_DECODE_BATCH // n
        for c, b0 in enumerate(range(0, B, per)):
            ns = min(per, B - b0)                          # segments of this decode batch, n rows each
            nb = ns * n
            dec = _decoder_for(model, nb, max_length, Le)
            enc_c = enc.view(B, Le, d)[b0:b0 + ns].reshape(ns * Le, d)
            ckv = dec.cross_kv(enc_c, ns, Le) if n == 1 else dec.cross_kv_beam(enc_c, ns, n, Le)
            toks, done, fin, *lp = dec.run(ckv, nb, Le, max_length, poll_every, ban=dec.ban_mask(bad_token_ids),
                                           return_logprobs=return_logprobs,
                                           sampling=sampling.shifted(c) if sampling else None)
            steps = (fin + 1) if fin >= 0 else max_length
            out.append((toks[:nb, :steps + 1].clone(), steps, lp[0][:nb, :steps + 1].clone() if lp else None))
        if len(out) == 1:
            return _pair(out[0][0], out[0][2], return_logprobs)
        # the reference stops when ALL rows are finished: pad shorter groups with pad_token_id
        steps = max(s for _, s, _ in out)
        res = torch.full((B * n, steps + 1), cfg["pad_token_id"], dtype=torch.int64, device=inputs.device)
        res_lp = torch.zeros(B * n, steps + 1, dtype=torch.float32, device=inputs.device) if return_logprobs else None
        r = 0
        for t, s, lp in out:
            res[r:r + t.shape[0], :s + 1] = t
            if return_logprobs:
                res_lp[r:r + t.shape[0], :s + 1] = lp
            r += t.shape[0]
        return _pair(res, res_lp, return_logprobs)
    if model.VARIANT == "segmem_v1":
        raise RuntimeError("T5SegMem.generate is the plain batched decode; memory decode is generate_2")
    # segment-memory models: sequential segments, memory = previous segment's tokens
    Ls = min(model.segmem_length, max_length)            # `[:, :segmem_length]` of a max_length-long sequence
    seg_ids = torch.zeros(1, max_length, dtype=torch.int64, device=inputs.device)
    if model.VARIANT == "segmem_v2_with_prev":
        seg_ids[0, 0], seg_ids[0, 1] = 1134, 1          # tie token + EOS (t5_segmem_v2_with_prev.py:257-258)
    else:
        seg_ids[0, 0] = 1                                # t5_segmem_v2.py:199
    dec = _decoder_for(model, 1, max_length, Le + Ls)
    outs, outs_lp = [], []
    for i in range(B):
        mem = _memory(eng, seg_ids, 1, max_length, Ls)                     # [1, Ls, d]
        cur = torch.cat([enc.view(B, Le, d)[i:i + 1], mem], 1).contiguous().view(Le + Ls, d)
        ckv = dec.cross_kv(cur, 1, Le + Ls)
        toks, done, fin, *lp = dec.run(ckv, 1, Le + Ls, max_length, poll_every, ban=dec.ban_mask(bad_token_ids),
                                       return_logprobs=return_logprobs,
                                       sampling=sampling.shifted(i) if sampling else None)
        steps = (fin + 1) if fin >= 0 else max_length
        row = torch.zeros(1, max_length, dtype=torch.int64, device=inputs.device)
        n = min(steps + 1, max_length)                   # F.pad(..., max_length - len) truncates (:287-291)
        row[0, :n] = toks[0, :n]
        outs.append(row)
        if lp:
            outs_lp.append(_logp_rows(lp[0][:1, :n], max_length))
        seg_ids = row
    return _pair(torch.cat(outs, 0), torch.cat(outs_lp, 0) if outs_lp else None, return_logprobs)


def _memory(eng, seg_ids, B, L, Ls):
    """Memory vectors of the previous segment; `segmem_length=0` (the reference's no-memory ablation,
    `[:, :0]`) yields an empty block without touching the memory encoder."""
    if Ls == 0:
        return torch.empty(B, 0, eng.d, device=seg_ids.device, dtype=eng.dt)
    return eng.segmem(seg_ids, B, L)


@torch.no_grad()
def generate_2(model, inputs, max_length=1024, poll_every=64, num_beams=1, return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0):
    """`T5SegMem.generate_2` (models/t5_segmem.py:172-252): segments one after the other; the previous
    segment's tokens go through the segment-memory encoder and its first `segmem_length` outputs are
    PREPENDED to the decoder's input embeddings.  With the KV cache that is a prefix fill: the memory
    rows are fed as decoder positions 0..Ls-1 (self-attention K/V only), tokens start at position Ls.
    A stable prefix buffer keeps the captured step graph valid across segments.  No beam search here.
    `do_sample`: the token steps draw (segment i with `seed + i`), the prefix steps draw nothing."""
    if num_beams != 1:
        raise ValueError("generate_2 (memory-prefixed decode) has no beam search")
    sampling = _sampling(do_sample, temperature, top_k, top_p, seed)
    eng, cfg = model.engine, model.cfg
    if not inputs.is_cuda:
        raise RuntimeError("generate_2 needs device tensors (no CPU fallback)")
    Ls = model.segmem_length
    assert max_length >= Ls, "the reference asserts segmem_length memory rows (t5_segmem.py:213)"
    eng.prepare(False)
    B, Le, d = inputs.shape
    enc = eng.encode(inputs)
    seg_ids = torch.zeros(1, max_length, dtype=torch.int64, device=inputs.device)
    seg_ids[0, 0] = 1                                          # t5_segmem.py:190-196
    dec = _decoder_for(model, 1, max_length + Ls, Le)
    pre = getattr(dec, "_prefix_buf", None)
    if pre is None or pre.shape[1] != Ls:
        pre = dec._prefix_buf = torch.empty(1, Ls, d, device=inputs.device, dtype=torch.float32)
    outs, outs_lp = [], []
    for i in range(B):
        if Ls:
            pre.copy_(eng.segmem(seg_ids, 1, max_length).float().view(1, Ls, d))
        ckv = dec.cross_kv(enc.view(B, Le, d)[i].contiguous(), 1, Le)
        toks, done, fin, *lp = dec.run(ckv, 1, Le, max_length, poll_every, prefix=pre if Ls else None,
                                       return_logprobs=return_logprobs,
                                       sampling=sampling.shifted(i) if sampling else None)
        steps = (fin + 1) if fin >= 0 else max_length
        row = torch.zeros(1, max_length, dtype=torch.int64, device=inputs.device)
        n = min(steps + 1, max_length)
        row[0, :n] = toks[0, :n]
        outs.append(row)
        if lp:
            outs_lp.append(_logp_rows(lp[0][:1, :n], max_length))
        seg_ids = row
    return _pair(torch.cat(outs, 0), torch.cat(outs_lp, 0) if outs_lp else None, return_logprobs)


@torch.no_grad()
def generate_songs(model, songs, max_length=1024, poll_every=64, num_beams=1, length_penalty=1.0, bad_token_ids=None,
                   return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0):
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
    eng, cfg = model.engine, model.cfg
    if model.VARIANT not in ("segmem_v2", "segmem_v2_with_prev"):
        raise RuntimeError("generate_songs is for the segment-memory models; plain T5 batches segments directly")
    if not songs:
        return _pair([], [], return_logprobs)
    per = MAX_DECODE_BATCH // num_beams
    if len(songs) > per:
        out, out_lp = [], []
        for i in range(0, len(songs), per):
            part = generate_songs(model, songs[i:i + per], max_length, poll_every, num_beams, length_penalty, bad_token_ids,
                                  return_logprobs, do_sample, temperature, top_k, top_p, seed)
            out += part[0] if return_logprobs else part
            out_lp += part[1] if return_logprobs else []
        return _pair(out, out_lp, return_logprobs)
    dev = songs[0].device
    if dev.type != "cuda":
        raise RuntimeError("generate_songs needs device tensors (no CPU fallback)")
    eng.prepare(False)
    S = len(songs)
    Le, d = songs[0].shape[1], songs[0].shape[2]
    Ls = min(model.segmem_length, max_length)
    enc = [eng.encode(x).view(x.shape[0], Le, d) for x in songs]           # per recording, all its segments
    first = torch.zeros(max_length, dtype=torch.int64, device=dev)
    if model.VARIANT == "segmem_v2_with_prev":
        first[0], first[1] = 1134, 1
    else:
        first[0] = 1
    prev = [first.clone() for _ in range(S)]
    outs = [[] for _ in range(S)]
    outs_lp = [[] for _ in range(S)]
    for i in range(max(x.shape[0] for x in songs)):
        live = [s for s in range(S) if i < songs[s].shape[0]]
        B = len(live)
        seg_ids = torch.stack([prev[s] for s in live])                      # [B, max_length]
        mem = _memory(eng, seg_ids, B, max_length, Ls)                     # [B, Ls, d]
        cur = torch.cat([torch.stack([enc[s][i] for s in live]), mem.to(enc[0].dtype)], 1).contiguous()
        dec = _decoder_for(model, B * num_beams, max_length, Le + Ls)
        if num_beams > 1:
            ckv = dec.cross_kv_beam(cur.view(B * (Le + Ls), d), B, num_beams, Le + Ls)
            ids, _, _, *lp = dec.run_beam(ckv, B, num_beams, Le + Ls, max_length, length_penalty,
                                          dec.ban_mask(bad_token_ids), poll_every, return_logprobs=return_logprobs)
            rows = _memory_rows(ids, max_length)
            rows_lp = _logp_rows(lp[0], max_length) if lp else None
        else:
            ckv = dec.cross_kv(cur.view(B * (Le + Ls), d), B, Le + Ls)
            toks, done, fin, *lp = dec.run(ckv, B, Le + Ls, max_length, poll_every, ban=dec.ban_mask(bad_token_ids),
                                           return_logprobs=return_logprobs,
                                           sampling=sampling.shifted(i) if sampling else None)
            rows = toks[:B, :max_length].clone()                           # finished rows are already pad(0)-filled
            rows_lp = lp[0][:B, :max_length].clone() if lp else None
            if done < max_length:                                          # all rows hit EOS early: the rest is stale
                rows[:, done + 1:] = 0
                if lp:
                    rows_lp[:, done + 1:] = 0
        for r, s in enumerate(live):
            outs[s].append(rows[r])
            if return_logprobs:
                outs_lp[s].append(rows_lp[r])
            prev[s] = rows[r]
    ids = [torch.stack(o) for o in outs]
    return (ids, [torch.stack(o) for o in outs_lp]) if return_logprobs else ids


def _check_beams(num_beams):
    if not (isinstance(num_beams, int) and 1 <= num_beams <= MAX_BEAMS):
        raise ValueError(f"num_beams must be an int in 1..{MAX_BEAMS}, got {num_beams!r}")


def _memory_rows(ids, max_length):
    """Beam output [n, W] -> [n, max_length]: cut or zero-padded, as the greedy chain does (`F.pad` / slice)."""
    rows = torch.zeros(ids.shape[0], max_length, dtype=torch.int64, device=ids.device)
    n = min(ids.shape[1], max_length)
    rows[:, :n] = ids[:, :n]
    return rows


def _logp_rows(logp, max_length):
    """`_memory_rows` for the log-probabilities that go with the ids: cut or padded with 0.0."""
    rows = torch.zeros(logp.shape[0], max_length, dtype=torch.float32, device=logp.device)
    n = min(logp.shape[1], max_length)
    rows[:, :n] = logp[:, :n]
    return rows


@torch.no_grad()
def generate_beam(model, inputs, num_beams=1, max_length=1024, length_penalty=1.0, bad_token_ids=None, poll_every=64,
                  return_logprobs=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0):
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
    if num_beams == 1:
        return _generate(model, inputs, max_length, poll_every, bad_token_ids, return_logprobs, sampling=sampling)
    eng, cfg = model.engine, model.cfg
    k = num_beams
    eng.prepare(False)
    B, Le, d = inputs.shape
    enc = eng.encode(inputs.float() if inputs.dtype not in (torch.float32, torch.bfloat16) else inputs)
    if model.VARIANT in ("t5", "segmem_v1"):
        per = MAX_DECODE_BATCH // k
        out = []
        for b0 in range(0, B, per):
            G = min(per, B - b0)
            dec = _decoder_for(model, G * k, max_length, Le)
            ckv = dec.cross_kv_beam(enc.view(B, Le, d)[b0:b0 + G].reshape(G * Le, d), G, k, Le)
            ids, _, _, *lp = dec.run_beam(ckv, G, k, Le, max_length, length_penalty, dec.ban_mask(bad_token_ids), poll_every,
                                          return_logprobs=return_logprobs)
            out.append((ids.clone(), lp[0].clone() if lp else None))
        if len(out) == 1:
            return _pair(out[0][0], out[0][1], return_logprobs)
        W = max(o.shape[1] for o, _ in out)
        res = torch.full((B, W), cfg["pad_token_id"], dtype=torch.int64, device=inputs.device)
        res_lp = torch.zeros(B, W, dtype=torch.float32, device=inputs.device) if return_logprobs else None
        r = 0
        for o, lp in out:
            res[r:r + o.shape[0], :o.shape[1]] = o
            if return_logprobs:
                res_lp[r:r + o.shape[0], :o.shape[1]] = lp
            r += o.shape[0]
        return _pair(res, res_lp, return_logprobs)
    Ls = min(model.segmem_length, max_length)
    seg_ids = torch.zeros(1, max_length, dtype=torch.int64, device=inputs.device)
    if model.VARIANT == "segmem_v2_with_prev":
        seg_ids[0, 0], seg_ids[0, 1] = 1134, 1
    else:
        seg_ids[0, 0] = 1
    dec = _decoder_for(model, k, max_length, Le + Ls)
    outs, outs_lp = [], []
    for i in range(B):
        mem = _memory(eng, seg_ids, 1, max_length, Ls)
        cur = torch.cat([enc.view(B, Le, d)[i:i + 1], mem], 1).contiguous().view(Le + Ls, d)
        ckv = dec.cross_kv_beam(cur, 1, k, Le + Ls)
        ids, _, _, *lp = dec.run_beam(ckv, 1, k, Le + Ls, max_length, length_penalty, dec.ban_mask(bad_token_ids), poll_every,
                                      return_logprobs=return_logprobs)
        row = _memory_rows(ids, max_length)
        outs.append(row)
        if lp:
            outs_lp.append(_logp_rows(lp[0], max_length))
        seg_ids = row
    return _pair(torch.cat(outs, 0), torch.cat(outs_lp, 0) if outs_lp else None, return_logprobs)
