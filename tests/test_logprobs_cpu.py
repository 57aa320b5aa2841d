"""Host side of the per-token log-probabilities: note confidences from a hand-written token stream with known
log-probabilities (two segments, one note tied across the boundary), `min_confidence`, and the unscored path unchanged."""
import math

import numpy as np
import pytest

from contrib import event_codec, metrics_utils, note_sequences, vocabularies
from contrib.note_sequences import Note

E = event_codec.Event


@pytest.fixture(scope="module")
def codec():
    return vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))


# (event, log-probability) per token.  Shifts count from the segment's start, in steps of 10 ms.
SEG1 = [                                  # starts at 0.0
    (E("tie", 0), -0.01),                 # empty tie section
    (E("shift", 10), -0.10),              # t = 0.10
    (E("velocity", 1), -0.02),
    (E("drum", 36), -0.05),               # drum: min(own -0.05, shift -0.10), no program token yet         -> exp(-0.10)
    (E("program", 5), -0.30),
    (E("velocity", 1), -0.02),
    (E("pitch", 60), -0.20),              # A on: min(own -0.20, program -0.30, shift -0.10)                 -> exp(-0.30)
    (E("shift", 20), -0.50),              # t = 0.20
    (E("program", 7), -0.03),
    (E("velocity", 1), -0.01),
    (E("pitch", 64), -0.04),              # B on: min(own -0.04, program -0.03, shift -0.50)                 -> exp(-0.50)
    (E("shift", 30), -0.02),              # t = 0.30
    (E("program", 7), -0.60),
    (E("velocity", 0), -0.01),
    (E("pitch", 64), -0.90),              # B off: the note keeps its onset's value
]
S2 = 1.024 - 1.024 % 0.01                 # the second segment's first frame time, rounded down to the codec step
SEG2 = [                                  # starts at S2 = 1.02
    (E("program", 5), -0.70),             # tie section: A is still sounding (these tokens do not touch A's value)
    (E("pitch", 60), -0.80),
    (E("tie", 0), -0.01),
    (E("shift", 50), -0.15),              # t = S2 + 0.50
    (E("velocity", 1), -0.01),
    (E("pitch", 67), -0.25),              # C on: min(own -0.25, this segment's program token -0.70, shift -0.15) -> exp(-0.70)
    (E("shift", 80), -0.05),              # t = S2 + 0.80
    (E("program", 5), -0.02),
    (E("velocity", 0), -0.01),
    (E("pitch", 60), -0.03),              # A off, with the confidence of its onset in segment 1
]                                         # C is closed by the final flush
WANT = {  # (pitch, is_drum) -> (start, end, program, confidence)
    (36, True): (0.10, 0.11, 0, math.exp(-0.10)),
    (64, False): (0.20, 0.30, 7, math.exp(-0.50)),
    (60, False): (0.10, S2 + 0.80, 5, math.exp(-0.30)),
    (67, False): (S2 + 0.50, S2 + 0.80, 5, math.exp(-0.70)),
}


def _arrays(codec, seg, width=20):
    """Post-processed token row and its log-probabilities as `InferenceHandler._postprocess_batch` leaves them: EOS = -1
    where the stream ends, padding after it."""
    tok = np.full(width, -1, dtype=np.int64)
    lp = np.zeros(width, dtype=np.float32)
    tok[:len(seg)] = [codec.encode_event(e) for e, _ in seg]
    lp[:len(seg)] = [p for _, p in seg]
    lp[len(seg)] = -0.001                 # the EOS token's own value: cut with it
    return tok, lp


def _handler(codec):
    import inference
    h = inference.InferenceHandler.__new__(inference.InferenceHandler)      # host methods only: no model, no device
    h.codec = codec
    return h


def _inputs(codec):
    t1, l1 = _arrays(codec, SEG1)
    t2, l2 = _arrays(codec, SEG2)
    frame_times = [np.stack([np.arange(256) * 0.008, 1.024 + np.arange(256) * 0.008])]
    return [np.stack([t1, t2])], frame_times, [np.stack([l1, l2])]


def test_note_confidence_follows_the_rule(codec):
    toks, ft, lps = _inputs(codec)
    ns = _handler(codec)._to_event(toks, ft, lps)
    assert len(ns.notes) == len(WANT)
    for n in ns.notes:
        start, end, program, conf = WANT[(n.pitch, n.is_drum)]
        assert n.start_time == pytest.approx(start) and n.end_time == pytest.approx(end)
        assert n.program == program
        assert n.confidence == pytest.approx(conf, rel=1e-6), (n, conf)
    by_pitch = {n.pitch: n for n in ns.notes}
    assert by_pitch[64].instrument == 0 and by_pitch[60].instrument == 1 and by_pitch[36].instrument == 9


@pytest.mark.parametrize("floor,kept", [(0.45, {36, 64, 60, 67}), (0.6, {36, 64, 60}), (0.7, {36, 60}), (0.95, set())])
def test_min_confidence_drops_exactly_the_notes_below_it(codec, floor, kept):
    toks, ft, lps = _inputs(codec)
    ns = _handler(codec)._to_event(toks, ft, lps, min_confidence=floor)
    assert {n.pitch for n in ns.notes} == kept
    if floor == 0.7:                      # instruments are assigned among the notes that stay
        assert {n.pitch: n.instrument for n in ns.notes} == {36: 9, 60: 0}


def test_unscored_decode_is_unchanged_and_scored_notes_equal_it(codec):
    toks, ft, lps = _inputs(codec)
    h = _handler(codec)
    plain = h._to_event(toks, ft)
    # today's path, spelled out: the reference's spec through event_predictions_to_ns
    preds = [{"est_tokens": t[:np.argmax(t == -1)], "start_time": s, "raw_inputs": []} for t, s in zip(toks[0], (0.0, S2))]
    today = metrics_utils.event_predictions_to_ns(preds, codec=codec, encoding_spec=note_sequences.NoteEncodingWithTiesSpec)
    assert plain.notes == today["est_ns"].notes and plain.total_time == today["est_ns"].total_time
    assert all(n.confidence == 1.0 for n in plain.notes)
    scored = h._to_event(toks, ft, lps)
    assert scored.notes == plain.notes and scored.total_time == plain.total_time      # confidence is not identity
    assert any(n.confidence != 1.0 for n in scored.notes)
    res = metrics_utils.event_predictions_to_ns_scored(
        [dict(p, est_logprobs=l[:len(p["est_tokens"])]) for p, l in zip(preds, lps[0])], codec=codec,
        encoding_spec=note_sequences.NoteEncodingWithTiesScoredSpec)
    assert res["est_invalid_events"] == today["est_invalid_events"] == 0
    assert res["est_dropped_events"] == today["est_dropped_events"] == 0


def test_note_construction_and_equality_ignore_confidence():
    assert Note(0, 1, 60, 100) == Note(0, 1, 60, 100)
    a, b = Note(0, 1, 60, 100, confidence=0.25), Note(0, 1, 60, 100, confidence=0.75)
    assert a == b and a.confidence != b.confidence
    assert Note(0, 1, 60, 100, 3, True, 9) == Note(0, 1, 60, 100, program=3, is_drum=True, instrument=9)
    assert Note(0, 1, 60, 100).confidence == 1.0 and Note(0, 1, 61, 100) != Note(0, 1, 60, 100)


def test_decode_events_and_decode_note_event_keep_their_signatures(codec):
    """The unscored entry points are callable exactly as before; the scored siblings take the per-token array."""
    from contrib import run_length_encoding
    tokens = [codec.encode_event(e) for e, _ in SEG1]
    st = note_sequences.NoteDecodingState()
    note_sequences.begin_tied_pitches_section(st)
    assert run_length_encoding.decode_events(st, tokens, 0.0, None, codec, note_sequences.decode_note_event) == (0, 0)
    st2 = note_sequences.ScoredNoteDecodingState()
    note_sequences.begin_tied_pitches_section_scored(st2)
    assert run_length_encoding.decode_events_scored(st2, tokens, [p for _, p in SEG1], 0.0, None, codec,
                                                    note_sequences.decode_note_event_scored) == (0, 0)
    assert note_sequences.flush_note_decoding_state(st).notes == note_sequences.flush_note_decoding_state_scored(st2).notes
    with pytest.raises(AssertionError):
        run_length_encoding.decode_events_scored(st2, tokens, [0.0], 0.0, None, codec, note_sequences.decode_note_event_scored)
