"""Shared by tests/test_device_notes_{cpu,gpu}.py: the seeded corpus of token rows, the hand-written cases, the
host path they are all held to, and the comparison.

A case is one recording: `ids` [rows, ld] int64 MODEL ids with the start token in column 0 (what the decoder returns),
`logp` [rows, ld] float32 beside it, and `start` [rows] float64, the rows' start times.  The host path is the definition:
`inference.postprocess_batch` / `postprocess_logprobs`, the cut and the predictions exactly as `InferenceHandler._to_event`
builds them, then `metrics_utils.event_predictions_to_ns` (or `_scored`)."""
import dataclasses
import math
import types

import numpy as np
import torch

import inference
from contrib import metrics_utils, note_sequences, vocabularies

CODEC = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
V = vocabularies.vocab_size(CODEC)               # 1491
SP = vocabularies.NUM_SPECIAL_TOKENS
PAD, EOS, UNK = 0, 1, 2
_lo = {t: CODEC.event_type_range(t)[0] + SP for t in ("shift", "pitch", "velocity", "tie", "program", "drum")}
OFF, ON, TIE = _lo["velocity"], _lo["velocity"] + 1, _lo["tie"]
FIRST_UNUSED = SP + CODEC.num_classes            # the first id past the codec: an extra id


def S(v): return _lo["shift"] + v
def P(p): return _lo["pitch"] + p
def G(p): return _lo["program"] + p
def D(p): return _lo["drum"] + p


@dataclasses.dataclass
class Case:
    name: str
    ids: np.ndarray
    logp: np.ndarray
    start: np.ndarray
    expect: dict = None                          # hand-written cases: the known answer
    frames: np.ndarray = None                    # the rows' first frame times, where `start` was derived from them


def frame_starts(n_rows, frames=256, fps=125.0):
    """The rows' first frame times as `inference.audio_to_frames` + `split_into_segments` give them."""
    return np.arange(n_rows * frames)[::frames] / fps


def row_start(t, codec=CODEC):
    """`_to_event`'s start time of a row whose first frame is at `t`."""
    t = np.float64(t)
    t -= t % (1 / codec.steps_per_second)
    return t


def _case(name, rows, rng, start=None, expect=None, ld=None):
    """rows: token id lists without the start column; padded with PAD to a common width."""
    width = max([len(r) for r in rows] + [1])
    ld = ld or width + 1
    ids = np.full((len(rows), ld), PAD, np.int64)
    for i, r in enumerate(rows):
        ids[i, 1:1 + min(len(r), ld - 1)] = r[:ld - 1]
    logp = -rng.exponential(1.0, size=ids.shape).astype(np.float32)
    frames = None
    if start is None:
        frames = frame_starts(len(rows))
        start = [row_start(t) for t in frames]
    return Case(name, ids, logp, np.asarray(start, np.float64), expect, frames)


# ---- the corpus ---------------------------------------------------------------------------------------------------------
PROGRAMS, PITCHES = (0, 25, 40), tuple(range(55, 67))
MUTANTS = (TIE, OFF, ON, S(3), S(150), PAD, UNK)


def _note_rows(rng, n_rows, events_of_row):
    """Note-like rows: a tie section declaring about 80 % of what sounds, then events at sorted random steps."""
    sounding, rows = [], []
    for r in range(n_rows):
        row = []
        keep = [k for k in sounding if rng.random_sample() < 0.8]
        for program, pitch in sorted(keep):
            row += [G(program), P(pitch)]
        row.append(TIE)
        sounding = keep
        steps = sorted(int(s) for s in rng.randint(0, 205, size=events_of_row(r)))
        cur = 0
        for s in steps:
            if s > cur:
                row.append(S(s))
                cur = s
            kind = rng.randint(3)
            if kind == 0:
                row += [ON, D(int(rng.randint(35, 50)))]
            elif kind == 1 and sounding:
                program, pitch = sounding.pop(int(rng.randint(len(sounding))))
                row += [G(program), OFF, P(pitch)]
            else:
                key = (PROGRAMS[rng.randint(3)], PITCHES[rng.randint(12)])
                row += [G(key[0]), ON, P(key[1])]
                if key in sounding:
                    sounding.remove(key)
                sounding.append(key)
        rows.append(row)
    return rows


def corpus(n_cases=200, seed=20240):
    rng = np.random.RandomState(seed)
    out = []
    for c in range(n_cases):
        n_rows = (1, 2, 3, 7)[rng.randint(4)]
        n_events = (0, 1, 5, 20)[rng.randint(4)]
        rows = _note_rows(rng, n_rows, lambda r: n_events)
        rows = [row + [EOS] for row in rows]
        if rng.randint(10) == 0:
            rows[rng.randint(n_rows)].pop()      # one row without EOS: it contributes no tokens
        if c % 3 != 0:
            for row in rows:
                for j in range(len(row)):
                    u = rng.random_sample()
                    if u < 0.06:
                        row[j] = int(rng.randint(0, V + 8))
                    elif u < 0.10:
                        row[j] = MUTANTS[rng.randint(len(MUTANTS))]
        out.append(_case("corpus%03d" % c, rows, rng))
    return out


def dense_case(seed=7, n_rows=7, ld=1024):
    """One recording of `n_rows` rows filled to the last column."""
    rng = np.random.RandomState(seed)
    rows = [row[:ld - 2] + [EOS] for row in _note_rows(rng, n_rows, lambda r: 400)]
    assert all(len(row) == ld - 1 for row in rows)
    for row in rows:                             # a few stray tokens: shifts that follow shifts, offs and ties out of place
        for j in np.nonzero(rng.random_sample(ld - 2) < 0.03)[0]:
            row[j] = (TIE, OFF, ON, S(1))[rng.randint(4)]
    return _case("dense", rows, rng, ld=ld)


# ---- the hand-written cases: one per ValueError site, emission site and quirk ------------------------------------------
def hand_cases(seed=5):
    rng = np.random.RandomState(seed)
    two = [0.0, 2.04]
    mk = lambda name, rows, notes, invalid, dropped, start=None, **more: _case(
        name, rows, rng, start=start, expect=dict(notes=notes, invalid=invalid, dropped=dropped, **more))
    cases = [
        mk("off", [[TIE, S(10), G(1), ON, P(60), S(50), OFF, P(60), EOS]], 1, 0, 0, times=[(0.1, 0.5)], programs=[1]),
        mk("re-onset then flush", [[TIE, S(10), ON, P(60), S(20), P(60), EOS]], 2, 0, 0, times=[(0.1, 0.2), (0.2, 0.2 + 0.01)]),
        mk("drum", [[TIE, ON, D(36), EOS]], 1, 0, 0, times=[(0.0, 0.01)], drums=[True]),
        mk("tie ends the undeclared, over an empty row", [[TIE, ON, P(60), P(62), EOS], [EOS], [G(0), P(60), TIE, EOS]],
           2, 0, 0, pitches=[62, 60]),
        mk("time < current time", [[TIE, S(50), ON, P(60), S(10), P(61), EOS]], 1, 1, 0, pitches=[60]),
        mk("inactive pitch in the tie section", [[G(0), P(60), TIE, EOS]], 0, 1, 0),
        mk("note-off for an inactive pitch", [[TIE, OFF, P(60), EOS]], 0, 1, 0),
        mk("drum at velocity zero", [[TIE, OFF, D(36), EOS]], 0, 1, 0),
        mk("tie outside the tie section", [[TIE, TIE, EOS]], 0, 1, 0),
        mk("a row without EOS", [[TIE, ON, P(60)]], 0, 0, 0),
        mk("UNK cuts like EOS", [[TIE, ON, P(60), UNK, P(61), EOS]], 1, 0, 0, pitches=[60]),
        mk("PAD is an invalid event", [[TIE, PAD, ON, P(60), EOS]], 1, 1, 0),
        mk("ids past the codec", [[TIE, FIRST_UNUSED, V + 5, ON, P(60), EOS]], 1, 2, 0),
        mk("a shift exactly onto the limit", [[TIE, S(204), ON, D(36), EOS], [TIE, EOS]], 1, 0, 0, start=two),
        mk("a shift one step past the limit", [[TIE, S(205), ON, D(36), EOS], [TIE, EOS]], 0, 0, 3, start=two),
        mk("no limit", [[TIE, S(1000), ON, D(40), EOS]], 1, 0, 0, times=[(10.0, 10.0 + 0.01)]),
        mk("a re-struck key moves to the end", [[TIE, ON, P(60), P(62), S(10), P(60), EOS]], 3, 0, 0, pitches=[60, 62, 60]),
        mk("a shift run longer than a chunk of the kernel's", [[TIE] + [S(1)] * 300 + [ON, D(36)] + [S(1)] * 300 + [ON, D(37), EOS]],
           2, 0, 0, times=[(3.0, 3.0 + 0.01), (3.0, 3.0 + 0.01)]),
    ]
    for pitch in (60, 61, 62, 63, 64):                 # "already tied" is rare in the corpus
        cases.append(mk("already tied %d" % pitch, [[TIE, ON, P(pitch), EOS], [P(pitch), P(pitch), TIE, EOS]], 1, 1, 0))
    return cases


def check_expectation(case, arrays):
    e = case.expect
    assert (len(arrays), arrays.invalid, arrays.dropped) == (e["notes"], e["invalid"], e["dropped"]), \
        (case.name, len(arrays), arrays.invalid, arrays.dropped, e)
    if "times" in e:
        assert [tuple(t) for t in arrays.times.tolist()] == [tuple(map(float, t)) for t in e["times"]], (case.name, arrays.times)
    if "pitches" in e:
        assert arrays.meta[:, 0].tolist() == e["pitches"], (case.name, arrays.meta)
    if "programs" in e:
        assert (arrays.meta[:, 2] & 0xff).tolist() == e["programs"], case.name
    if "drums" in e:
        assert (arrays.meta[:, 2] >> 8 & 1).astype(bool).tolist() == e["drums"], case.name


# ---- the host path ------------------------------------------------------------------------------------------------------
def predictions(case, scored):
    """The predictions `_to_event` hands to `event_predictions_to_ns`, from the case's start times."""
    tokens = inference.postprocess_batch(torch.from_numpy(case.ids), EOS)
    lps = inference.postprocess_logprobs(torch.from_numpy(case.logp))
    out = []
    for j, row in enumerate(tokens):
        n = np.argmax(row == vocabularies.DECODED_EOS_ID)
        out.append({"est_tokens": row[:n], "start_time": case.start[j], "raw_inputs": []})
        if scored:
            out[-1]["est_logprobs"] = lps[j][:n]
    return out


class ExpSpy:
    """Stands in for `math` inside contrib.note_sequences: records what `exp` is given, the value a note holds before it."""

    def __init__(self):
        self.seen = []

    def exp(self, x):
        self.seen.append(x)
        return math.exp(x)

    def __getattr__(self, name):
        return getattr(math, name)


def host_path(case, scored=False, min_confidence=None, spec=None, monkeypatch=None):
    """(note sequence, invalid, dropped, the pre-exp values in note order or None)."""
    if not scored:
        spec = spec or note_sequences.NoteEncodingWithTiesSpec
        r = metrics_utils.event_predictions_to_ns(predictions(case, False), codec=CODEC, encoding_spec=spec)
        return r["est_ns"], r["est_invalid_events"], r["est_dropped_events"], None
    spy = ExpSpy()
    monkeypatch.setattr(note_sequences, "math", spy)
    r = metrics_utils.event_predictions_to_ns_scored(predictions(case, True), codec=CODEC,
                                                     encoding_spec=note_sequences.NoteEncodingWithTiesScoredSpec,
                                                     min_confidence=min_confidence)
    monkeypatch.setattr(note_sequences, "math", math)
    return r["est_ns"], r["est_invalid_events"], r["est_dropped_events"], spy.seen


def to_event(case, scored=False, min_confidence=None):
    """`InferenceHandler._to_event` itself on the case's frame times."""
    stub = types.SimpleNamespace(codec=CODEC)
    tokens = inference.postprocess_batch(torch.from_numpy(case.ids), EOS)
    lps = [inference.postprocess_logprobs(torch.from_numpy(case.logp))] if scored else None
    return inference.InferenceHandler._to_event(stub, [tokens], [case.frames[:, None].copy()], lps, min_confidence)


def limits(start):
    lim = np.zeros(len(start), np.float64)
    lim[:-1] = start[1:]
    return lim


def bits64(a): return np.ascontiguousarray(a, np.float64).view(np.uint64)
def bits32(a): return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_as_host(arrays, ns, invalid, dropped, pre_exp, what):
    """`arrays` (a NoteArrays) against the host path's result, every field; f64 times and f32 scores bit for bit."""
    assert (arrays.invalid, arrays.dropped) == (invalid, dropped), (what, arrays.invalid, arrays.dropped, invalid, dropped)
    assert len(arrays) == len(ns.notes), (what, len(arrays), len(ns.notes))
    want_t = np.asarray([(n.start_time, n.end_time) for n in ns.notes], np.float64).reshape(-1, 2)
    want_m = np.asarray([(n.pitch, n.velocity, n.program | int(n.is_drum) << 8, 0) for n in ns.notes], np.int32).reshape(-1, 4)
    assert np.array_equal(bits64(arrays.times), bits64(want_t)), (what, arrays.times, want_t)
    assert np.array_equal(arrays.meta, want_m), (what, arrays.meta, want_m)
    assert bits64([arrays.total_time])[0] == bits64([ns.total_time])[0], (what, arrays.total_time, ns.total_time)
    mine = arrays.to_note_sequence()
    assert mine.notes == ns.notes and [n.instrument for n in mine.notes] == [n.instrument for n in ns.notes], what
    assert type(mine) is type(ns) and mine.total_time == ns.total_time and mine.ticks_per_quarter == ns.ticks_per_quarter
    if pre_exp is not None:
        assert arrays.logc.dtype == np.float32
        assert np.array_equal(bits32(arrays.logc), bits32(np.asarray(pre_exp, np.float64))), (what, arrays.logc, pre_exp)
        assert all(np.float32(x) == x for x in pre_exp), what           # the host's values ARE f32 values
        assert [n.confidence for n in mine.notes] == [n.confidence for n in ns.notes], what
    else:
        assert arrays.logc is None


def same_arrays(got, want, what):
    """Two NoteArrays, field for field (the kernel against `decode_notes_host`)."""
    assert (got.status, got.invalid, got.dropped, len(got)) == (want.status, want.invalid, want.dropped, len(want)), \
        (what, got.status, got.invalid, got.dropped, len(got), want.status, want.invalid, want.dropped, len(want))
    assert np.array_equal(bits64(got.times), bits64(want.times)), (what, got.times, want.times)
    assert np.array_equal(got.meta, want.meta), (what, got.meta, want.meta)
    assert bits64([got.total_time])[0] == bits64([want.total_time])[0], (what, got.total_time, want.total_time)
    assert (got.logc is None) == (want.logc is None), what
    if want.logc is not None:
        assert np.array_equal(bits32(got.logc), bits32(want.logc)), (what, got.logc, want.logc)


def grammar():
    from mrmt3.grammar import EventGrammar
    return EventGrammar.from_codec(CODEC)


def host_arrays(case, scored):
    from mrmt3 import notes
    return notes.decode_notes_host(grammar(), case.ids, np.asarray([0, len(case.ids)], np.int32), case.start,
                                   limits(case.start), notes.velocity_table(CODEC), CODEC.steps_per_second,
                                   case.logp if scored else None)[0]
