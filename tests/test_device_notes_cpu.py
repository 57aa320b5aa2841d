"""Token rows -> notes without a GPU: `mrmt3.notes.decode_notes_host`, the host restatement of the row contract
of `mrmt3_notes_decode_fwd`, is held to the definition — `_postprocess_batch` + `_to_event` + `event_predictions_to_ns` (or
`_scored`) — over the seeded corpus and the hand-written cases of tests/_notes.py: every note field with f64 times bit for
bit and in order, `instrument`, `total_time`, `invalid`, `dropped`, and scored the value before `exp` as f32 bit for bit.
The test asserts its own coverage: a spy around `decode_note_event` must see every ValueError site and every emission site."""
import collections
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _notes as N  # noqa: E402
from contrib import metrics_utils, note_sequences, vocabularies  # noqa: E402

ERROR_SITES = ("event time < current time", "inactive pitch/program in tie section", "pitch/program is already tied",
               "note-off for inactive pitch/program", "velocity cannot be zero for drum event",
               "tie section end event when not in tie section")
EMISSION_SITES = ("off", "re-onset", "drum", "tie", "flush")


@pytest.fixture(scope="module")
def cases():
    return N.corpus() + N.hand_cases()


class Spy:
    """`decode_note_event` and the flush, counted by the site that raised or emitted."""

    def __init__(self):
        self.seen = collections.Counter()
        self.spec = note_sequences.NoteEncodingSpecType(note_sequences.NoteDecodingState,
                                                        note_sequences.begin_tied_pitches_section, self.event, self.flush)

    def event(self, state, time, event, codec):
        before, velocity, tie_section = len(state.note_sequence.notes), state.current_velocity, state.is_tie_section
        try:
            note_sequences.decode_note_event(state, time, event, codec)
        except ValueError as e:
            site = [s for s in ERROR_SITES if str(e).startswith(s)]
            assert len(site) == 1, str(e)
            self.seen[site[0]] += 1
            raise
        if len(state.note_sequence.notes) > before:
            assert not tie_section or event.type in ("tie", "drum")
            self.seen["drum" if event.type == "drum" else "tie" if event.type == "tie" else
                      "off" if velocity == 0 else "re-onset"] += 1

    def flush(self, state):
        if state.active_pitches:
            self.seen["flush"] += 1
        return note_sequences.flush_note_decoding_state(state)


def test_host_restatement_equals_the_host_path(cases, monkeypatch):
    """Unscored and scored, every case; the spy's counts are a condition of the test."""
    spy = Spy()
    notes = tokens = 0
    for case in cases:
        ns, invalid, dropped, _ = N.host_path(case, spec=spy.spec)
        got = N.host_arrays(case, scored=False)
        N.same_as_host(got, ns, invalid, dropped, None, case.name)
        if case.expect is not None:
            N.check_expectation(case, got)
        ns, invalid, dropped, pre_exp = N.host_path(case, scored=True, monkeypatch=monkeypatch)
        N.same_as_host(N.host_arrays(case, scored=True), ns, invalid, dropped, pre_exp, case.name + " scored")
        notes += len(ns.notes)
        tokens += case.ids.size
    print("[device notes] %d cases, %d ids, %d notes, sites %s" % (len(cases), tokens, notes, dict(spy.seen)))
    for site in ERROR_SITES + EMISSION_SITES:
        assert spy.seen[site] >= 3, (site, dict(spy.seen))


def test_to_event_itself_gives_the_same_notes(cases):
    """The predictions tests/_notes.py builds are `_to_event`'s: the method itself, on the frame times, returns the notes."""
    for case in [c for c in cases if c.frames is not None][::7]:
        assert N.to_event(case).notes == N.host_path(case)[0].notes, case.name
        assert N.to_event(case, scored=True, min_confidence=0.3).notes == N.host_arrays(case, True).to_note_sequence(0.3).notes


def test_min_confidence_equals_the_scored_flush(cases, monkeypatch):
    """`to_note_sequence(min_confidence=)`: the notes `flush_note_decoding_state_scored` keeps under the same floor, their
    instruments assigned among the kept."""
    dropped_some = 0
    for case in cases:
        arrays = N.host_arrays(case, scored=True)
        for floor in (0.2, 0.5):
            ns = N.host_path(case, scored=True, min_confidence=floor, monkeypatch=monkeypatch)[0]
            mine = arrays.to_note_sequence(min_confidence=floor)
            assert mine.notes == ns.notes and mine.total_time == ns.total_time, (case.name, floor)
            assert [(n.instrument, n.confidence) for n in mine.notes] == [(n.instrument, n.confidence) for n in ns.notes]
            dropped_some += len(ns.notes) < len(arrays)
    assert dropped_some > 20
    with pytest.raises(ValueError, match="scored"):
        N.host_arrays(cases[0], scored=False).to_note_sequence(min_confidence=0.5)


def test_segment_times_equal_what_to_event_and_the_combiner_derive(monkeypatch):
    """seg_first / start_time / limit from frame times: `_to_event`'s start of every row and the limit
    `decode_and_combine_predictions` hands to the decoder (None = 0.0), for real frame times of several recordings."""
    import types

    import inference
    from mrmt3 import notes
    seen = []

    def capture(predictions, codec, encoding_spec):
        def decode(state, tokens, start_time, limit):
            seen.append((start_time, limit))
            return 0, 0
        metrics_utils.decode_and_combine_predictions(predictions, encoding_spec.init_decoding_state_fn,
                                                     encoding_spec.begin_decoding_segment_fn, decode,
                                                     encoding_spec.flush_decoding_state_fn)
        return {"est_ns": None}

    monkeypatch.setattr(metrics_utils, "event_predictions_to_ns", capture)
    stub = types.SimpleNamespace(codec=N.CODEC)
    lengths = (1, 16000 * 3 + 5, 16000 * 41, 128 * 256 * 3)
    all_ft, want = [], []
    for n in lengths:
        frames, times = inference.audio_to_frames(np.zeros(n, np.float32))
        _, ft, _ = inference.split_into_segments(frames, times)
        del seen[:]
        inference.InferenceHandler._to_event(stub, [np.full((len(ft), 4), -1)], [ft])
        assert len(seen) == len(ft)
        all_ft.append(ft)
        want.append(list(seen))
    seg_first, start, limit, order = notes.segment_times(np.concatenate(all_ft), N.CODEC, [len(ft) for ft in all_ft])
    assert order is None and seg_first.dtype == np.int32 and seg_first.tolist() == np.cumsum([0] + [len(f) for f in all_ft]).tolist()
    flat = [x for rec in want for x in rec]
    assert N.bits64(start).tolist() == N.bits64([s for s, _ in flat]).tolist()
    assert N.bits64(limit).tolist() == N.bits64([0.0 if m is None else m for _, m in flat]).tolist()
    assert (limit[seg_first[1:] - 1] == 0).all() and (limit > 0).sum() == len(limit) - len(lengths)
    # rows out of time order are put in order, as the combiner's stable sort does
    _, start2, _, order2 = notes.segment_times(all_ft[2][::-1], N.CODEC)
    assert order2.tolist() == list(range(len(all_ft[2])))[::-1] and (np.diff(start2) > 0).all()
    with pytest.raises(ValueError, match="add up"):
        notes.segment_times(all_ft[1], N.CODEC, [1])


def test_arguments_the_host_refuses():
    from mrmt3 import notes
    from mrmt3.grammar import EventGrammar
    case = N.hand_cases()[0]
    g, vel = N.grammar(), notes.velocity_table(N.CODEC)
    assert vel.tolist() == [0, 127] and g.steps_per_second == 100 and g.c_struct().steps_per_second == 100
    args = lambda **kw: {**dict(grammar=g, ids=case.ids, seg_first=[0, 1], start_time=case.start, limit=N.limits(case.start),
                                velocity_of_bin=vel, steps_per_second=100), **kw}
    assert len(notes.decode_notes_host(**args())[0]) == 1
    for bad in (dict(seg_first=[0, 2]), dict(seg_first=[1, 1]), dict(seg_first=[0]), dict(ids=case.ids[:, :1]),
                dict(steps_per_second=0), dict(steps_per_second=62.5), dict(grammar=dataclasses.replace(g, n_program=129))):
        with pytest.raises(ValueError):
            notes.decode_notes_host(**args(**bad))
    # a codec other than build_codec's is refused by name
    from contrib import event_codec
    other = event_codec.Codec(1000, 100, [event_codec.EventRange("pitch", 0, 127), event_codec.EventRange("velocity", 0, 1)])
    with pytest.raises(ValueError, match="build_codec"):
        notes.check_codec(other)
    notes.check_codec(vocabularies.build_codec(vocabularies.VocabularyConfig()))
    assert EventGrammar.from_codec(vocabularies.build_codec(vocabularies.VocabularyConfig(steps_per_second=50))).steps_per_second == 50


def test_binding_and_the_handler_keyword():
    """The symbols exist with the header's signatures, the capacity is the ABI's, a CPU tensor is an error, and the handler
    takes the keyword (off by default)."""
    import inspect
    import re

    import torch

    import inference
    from mrmt3 import lib, notes
    so = lib.load()
    assert so.mrmt3_version() >= 126 and lib.MIN_VERSION >= 126
    assert {"mrmt3_notes_decode_fwd", "mrmt3_notes_launches"} <= set(lib.header_symbols())
    assert int(re.search(r"#define MRMT3_NOTES_CAPACITY (\d+)", open(lib.HEADER_PATH).read()).group(1)) == lib.NOTES_CAPACITY >= 2048
    before = lib.notes_launches()
    with pytest.raises(RuntimeError, match="device"):
        notes.decode_notes(torch.zeros(2, 8, dtype=torch.int64), np.zeros((2, 256)), N.CODEC)
    assert lib.notes_launches() == before
    for fn in (inference.InferenceHandler.__init__, inference.InferenceHandler.inference, inference.InferenceHandler.inference_many):
        assert "device_notes" in inspect.signature(fn).parameters
    assert inspect.signature(inference.InferenceHandler.__init__).parameters["device_notes"].default is False
