"""TEST INFRASTRUCTURE ONLY: host restatement of the MT3 event grammar the decoder enforces on the device (csrc/decode_grammar.hip
`gram_push` / `gram_allowed`), next to tests/beam_ref.py and tests/sample_ref.py.  Plain Python sets and numpy;
nothing here shares code with the kernel or with mrmt3/grammar.py: the id ranges come from the codec, the rules from the table.

Per-row state: `mode` ("tie" / "body"), `program` (None = unset), `velocity` (None / "off" / "on"), `cur` (step time of the last
non-shift event), `acc` (steps of the running shift run), `active` (set of (program, pitch)) and the read-only `carry`.

  token      tie section                                            body
  pad/unk/non-event  never                                          never
  EOS        no                                                     yes
  tie        yes -> body, active = the set just declared            no
  program p  yes, sets program                                      yes, sets program
  velocity   no                                                     yes, sets velocity (first id = off, the others = on)
  pitch k    program set, (program, k) not declared yet and,        program and velocity set; on: any k, sets the bit;
             with a carry, in it; sets the bit                      off: only an active (program, k), clears the bit
  drum k     no                                                     velocity on
  shift v    no                                                     v >= 1 and cur < acc + v <= max_shift_steps; acc += v
Any non-shift token taken in the body sets cur = max(cur, acc), then acc = 0.
"""
import math

import numpy as np

from contrib import note_sequences, run_length_encoding, spectrograms, vocabularies

SPECIAL = vocabularies.NUM_SPECIAL_TOKENS
EOS, PAD = 1, 0


def default_max_shift_steps(codec, mel_length=256, spectrogram_config=None):
    """The largest step count `decode_events` keeps for a segment: times up to the next segment's start survive."""
    cfg = spectrogram_config or spectrograms.SpectrogramConfig()
    return int(math.floor(mel_length / cfg.frames_per_second * codec.steps_per_second + 1e-9))


class GrammarRef:
    def __init__(self, codec, V=None, max_shift_steps=None, tie_section=True, carry=None, ban=None):
        self.codec = codec
        self.V = V if V is not None else vocabularies.vocab_size(codec)
        self.rng = {n: tuple(x + SPECIAL for x in codec.event_type_range(n))          # inclusive model-id ranges
                    for n in ("shift", "pitch", "velocity", "tie", "program", "drum")}
        self.max_shift_steps = default_max_shift_steps(codec) if max_shift_steps is None else max_shift_steps
        self.ban = np.asarray(sorted({int(b) for b in (ban or ())}), dtype=np.int64)
        self.carry = None if carry is None else {(int(p), int(k)) for p, k in carry}
        self.mode = "tie" if tie_section else "body"
        self.program, self.velocity, self.cur, self.acc = None, None, 0, 0
        # a row without a tie section starts with what was sounding; with one it declares its own set
        self.active = set(self.carry) if (self.carry is not None and not tie_section) else set()

    def kind(self, tok):
        """(event type, value) of a model id, or (None, None) for pad / EOS / unk / ids outside the codec."""
        for n, (lo, hi) in self.rng.items():
            if lo <= tok <= hi:
                return n, tok - lo
        return None, None

    def allowed(self):
        a = np.zeros(self.V, dtype=bool)
        r = self.rng
        span = lambda n: slice(r[n][0], r[n][1] + 1)
        a[span("program")] = True
        if self.mode == "tie":
            a[r["tie"][0]] = True
            if self.program is not None:
                for k in range(r["pitch"][1] - r["pitch"][0] + 1):
                    key = (self.program, k)
                    if key not in self.active and (self.carry is None or key in self.carry):
                        a[r["pitch"][0] + k] = True
        else:
            a[EOS] = True
            a[span("velocity")] = True
            if self.velocity == "on":
                a[span("drum")] = True
            if self.program is not None and self.velocity is not None:
                if self.velocity == "on":
                    a[span("pitch")] = True
                else:
                    for p, k in self.active:
                        if p == self.program:
                            a[r["pitch"][0] + k] = True
            lo = max(1, self.cur - self.acc + 1)
            hi = min(self.max_shift_steps - self.acc, r["shift"][1] - r["shift"][0])
            if hi >= lo:
                a[r["shift"][0] + lo:r["shift"][0] + hi + 1] = True
        a[self.ban] = False
        return a

    def push(self, tok):
        n, v = self.kind(int(tok))
        if n == "shift":
            if self.mode == "body":
                self.acc += v
            return
        if self.mode == "tie":
            if n == "tie":
                self.mode = "body"
            elif n == "program":
                self.program = v
            elif n == "pitch" and self.program is not None:
                self.active.add((self.program, v))
            return
        self.cur, self.acc = max(self.cur, self.acc), 0
        if n == "program":
            self.program = v
        elif n == "velocity":
            self.velocity = "on" if v else "off"
        elif n == "pitch" and self.program is not None and self.velocity is not None:
            if self.velocity == "on":
                self.active.add((self.program, v))
            else:
                self.active.discard((self.program, v))

    def copy(self):
        c = GrammarRef.__new__(GrammarRef)
        c.__dict__.update(self.__dict__)
        c.active = set(self.active)
        return c


def set_to_bits(pairs):
    """{(program, pitch)} -> uint8 [2048]: bit program * 128 + pitch, least significant bit first."""
    b = np.zeros(2048, dtype=np.uint8)
    for p, k in pairs or ():
        i = p * 128 + k
        b[i >> 3] |= 1 << (i & 7)
    return b


def bits_to_set(bits):
    idx = np.flatnonzero(np.unpackbits(np.asarray(bits, dtype=np.uint8), bitorder="little"))
    return {(int(i) >> 7, int(i) & 127) for i in idx}


def random_carry(rs, n=24):
    """A few sounding notes over a few programs."""
    progs = rs.choice(128, size=4, replace=False)
    return {(int(rs.choice(progs)), int(rs.randint(0, 128))) for _ in range(n)}


def random_walk(codec, rs, steps, carry=None, **kw):
    """`steps` uniformly random allowed tokens from the start state.  -> (tokens, the GrammarRef after them).  Asserts the
    allowed set is never empty."""
    g = GrammarRef(codec, carry=carry, **kw)
    toks = []
    for _ in range(steps):
        a = np.flatnonzero(g.allowed())
        assert len(a) > 0, "empty allowed set"
        t = int(a[rs.randint(len(a))])
        toks.append(t)
        g.push(t)
        if t == EOS:
            break
    return toks, g


def count_invalid(tokens, carry, codec, tie_section=True, mel_length=256, spectrogram_config=None, time_limit=True):
    """(invalid, dropped) of the product's own `decode_events` + `decode_note_event` over a row's model ids (cut at the first
    EOS), on a note-decoding state seeded as the soundness condition says: its active set is `carry` or, without one, the
    row's own tie-section declarations.  `time_limit=False` decodes without the next segment's start as a limit: nothing is
    dropped, so every token of a row that shifts past the segment's end is still looked at."""
    cfg = spectrogram_config or spectrograms.SpectrogramConfig()
    toks = [int(t) for t in tokens]
    if EOS in toks:
        toks = toks[:toks.index(EOS)]
    state = note_sequences.NoteDecodingState()
    if carry is not None:
        seeded = set(carry)
    else:
        seeded, program = set(), None
        lo_p, hi_p = (x + SPECIAL for x in codec.event_type_range("program"))
        lo_k, hi_k = (x + SPECIAL for x in codec.event_type_range("pitch"))
        tie = codec.event_type_range("tie")[0] + SPECIAL
        for t in toks if tie_section else ():
            if t == tie:
                break
            if lo_p <= t <= hi_p:
                program = t - lo_p
            elif lo_k <= t <= hi_k and program is not None:
                seeded.add((program, t - lo_k))
    for p, k in seeded:
        state.active_pitches[(k, p)] = (0.0, note_sequences.DEFAULT_VELOCITY)
    if tie_section:
        note_sequences.begin_tied_pitches_section(state)
    return run_length_encoding.decode_events(state, np.asarray(toks, dtype=np.int64) - SPECIAL, 0.0,
                                             mel_length / cfg.frames_per_second if time_limit else None, codec,
                                             note_sequences.decode_note_event)


# ---- beam search under a mask per row ---------------------------------------------------------------------------------
from beam_ref import BeamRef  # noqa: E402


class MaskedBeamRef(BeamRef):
    """tests/beam_ref.py's search with `allowed` [G*k, V] bool per step in place of the static ban: a token a row may not
    emit scores -inf after the log-softmax, where the static ban acts."""

    def step(self, t, logits, allowed=None):
        if allowed is None:
            return super().step(t, logits)
        G, k, V = self.G, self.k, self.V
        x = np.asarray(logits, dtype=np.float64).reshape(G * k, V)
        m = x.max(-1, keepdims=True)
        logp = (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))
        # the base class bans whole columns; the rows' masks go in at the same place and the scorer walk below is the
        # base class's, line for line (without its margin bookkeeping)
        logp[~np.asarray(allowed, dtype=bool).reshape(G * k, V)] = -np.inf
        s = logp + self.scores[:, None]
        parents = np.arange(G * k)
        tokens = np.full(G * k, self.pad, dtype=np.int64)
        new = np.zeros(G * k)
        cur_len = t + 1
        for g in range(G):
            if self.done[g]:
                continue
            flat = s[g * k:(g + 1) * k].reshape(-1)
            order = np.lexsort((np.arange(flat.size), -flat))[:2 * k + 1]
            top = flat[order]
            nb = 0
            for rank in range(2 * k):
                c = int(order[rank])
                j, tok = divmod(c, V)
                if tok == self.eos:
                    if rank >= k:
                        continue
                    self._add(g, flat[c] / cur_len ** self.lp, t, g * k + j)
                else:
                    r = g * k + nb
                    parents[r], tokens[r], new[r] = g * k + j, tok, flat[c]
                    nb += 1
                if nb == k:
                    break
            assert nb == k
            if len(self.hyps[g]) >= k:
                self.done[g] = self.worst[g] >= top[0] / cur_len ** self.lp
        self.scores = new
        self.bp.append((parents, tokens))
        return parents, tokens, new
