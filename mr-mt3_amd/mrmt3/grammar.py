"""The MT3 event grammar for constrained decoding: which token may follow a row's history so that
`contrib.run_length_encoding.decode_events` + `contrib.note_sequences.decode_note_event` accept every token.

`EventGrammar` is the descriptor the device state machine reads (`mrmt3_grammar` of include/mrmt3_hip.h): the id ranges of a
codec in MODEL ids (the 3 special tokens included), the longest time a shift run may reach and whether a row starts in the tie
section.  The rules themselves live in csrc/decode_grammar.hip (`gram_push`, `gram_allowed`); tests/grammar_ref.py restates them on the
host.  `ACTIVE_BYTES` is the size of a row's `active` / `carry` bit set over (program, pitch): bit `program * 128 + pitch`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields

from contrib import spectrograms, vocabularies

ACTIVE_BYTES = 2048      # MRMT3_GRAMMAR_SET_BYTES


class _CGrammar(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("shift0", "n_shift", "pitch0", "n_pitch", "velocity0", "n_velocity", "tie", "program0",
                                       "n_program", "drum0", "n_drum", "eos", "pad", "max_shift_steps", "tie_section",
                                       "steps_per_second")]


@dataclass(frozen=True)
class EventGrammar:
    shift0: int
    n_shift: int
    pitch0: int
    n_pitch: int
    velocity0: int          # the note-off velocity; every other velocity id is "on"
    n_velocity: int
    tie: int
    program0: int
    n_program: int
    drum0: int
    n_drum: int
    eos: int
    pad: int
    max_shift_steps: int
    tie_section: bool = True
    steps_per_second: int = vocabularies.DEFAULT_STEPS_PER_SECOND   # read by the note decoder alone (mrmt3.notes)

    @classmethod
    def from_codec(cls, codec, mel_length=256, spectrogram_config=None, tie_section=True, max_shift_steps=None,
                   eos_token_id=1, pad_token_id=0):
        """The grammar of `codec` (`vocabularies.build_codec`).  `max_shift_steps` defaults to the largest step count
        `decode_events` keeps for a segment of `mel_length` frames: a shift run that reaches past the next segment's start
        drops the rest of the row.  That is floor(mel_length * hop / sample_rate * steps_per_second), 204 for 256 frames
        at 125 frames/s and 100 steps/s, and never more than the codec's own longest shift."""
        sp = vocabularies.NUM_SPECIAL_TOKENS

        def rng(name):
            lo, hi = codec.event_type_range(name)
            return lo + sp, hi - lo + 1

        if max_shift_steps is None:
            cfg = spectrogram_config or spectrograms.SpectrogramConfig()
            max_shift_steps = int(mel_length * cfg.hop_width * codec.steps_per_second) // int(cfg.sample_rate)
        max_shift_steps = int(max_shift_steps)
        if max_shift_steps < 0:
            raise ValueError(f"max_shift_steps must be >= 0, got {max_shift_steps}")
        (s0, ns), (p0, np_), (v0, nv), (t0, _), (g0, ng), (d0, nd) = (rng(n) for n in ("shift", "pitch", "velocity", "tie",
                                                                                      "program", "drum"))
        sps = codec.steps_per_second             # a grid that is not whole becomes 0, which the note decoder refuses
        return cls(s0, ns, p0, np_, v0, nv, t0, g0, ng, d0, nd, int(eos_token_id), int(pad_token_id), max_shift_steps,
                   bool(tie_section), int(sps) if sps == int(sps) and sps >= 1 else 0)

    def c_struct(self) -> _CGrammar:
        return _CGrammar(*[int(getattr(self, f.name)) for f in fields(self)])

    def check_ban(self, bad_token_ids) -> None:
        """`tie` (tie section) and EOS (body) are what keeps a row's allowed set from ever being empty: a static ban on
        either is refused."""
        bad = {int(i) for i in (bad_token_ids or ())}
        if self.eos in bad:
            raise ValueError("constrained decoding: bad_token_ids bans EOS, which would leave a row in the body with no allowed token")
        if self.tie_section and self.tie in bad:
            raise ValueError("constrained decoding: bad_token_ids bans the tie token, which would leave a row in the tie "
                             "section with no allowed token")


def resolve(constrained, model=None):
    """The `constrained` keyword of the entry points -> EventGrammar or None: False / None is off, True the default grammar
    of the inference codec (`num_velocity_bins=1`, 256-frame segments), an EventGrammar is used as given."""
    if constrained is None or constrained is False:
        return None
    if isinstance(constrained, EventGrammar):
        return constrained
    if constrained is True:
        cfg = getattr(model, "cfg", None) or {}
        codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
        return EventGrammar.from_codec(codec, eos_token_id=cfg.get("eos_token_id", 1), pad_token_id=cfg.get("pad_token_id", 0))
    raise TypeError(f"constrained must be a bool or an EventGrammar, got {type(constrained).__name__}")
