"""Frame scores, piano rolls and instrument detection without a GPU: the two host restatements of
`mrmt3_note_frames_fwd` against each other over the corpus of tests/_frame_cases.py and against the closed forms of the
hand-written cases, `evaluate.py`'s host path with the new options, the argument errors, and the library's symbols."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _frame_cases as F  # noqa: E402
import _note_match as M  # noqa: E402

TILE = 2048


def _both(packed, fps, n_frames):
    from mrmt3 import scoring
    dense = scoring.frame_counts_host(*packed.arrays(), fps, n_frames, with_roll=True)
    union = F.frame_counts_intervals(*packed.arrays(), fps, n_frames)
    for a, b in zip(dense[:3], union):
        assert a.dtype == b.dtype and (a == b).all(), np.argwhere(a != b)[:5]
    return dense


def test_dense_roll_equals_interval_union_on_the_corpus():
    cases = F.corpus()
    assert len(cases) >= 300 and any(not c[0] for c in cases) and any(not c[1] for c in cases)
    assert any(s == e for c in cases for s, e, _ in c[0])           # zero lengths occur
    packed = F.pack(cases)
    counts, skipped, clipped, roll = _both(packed, 62.5, 400)
    assert counts[:, 0].sum() > 10000 and (counts[:, 0] <= counts[:, 1:].min(1)).all()
    assert not skipped.any() and not clipped.any()
    # same-pitch overlaps occur: the union is smaller than the sum of the notes' frames
    from contrib import transcription_metrics as tm
    lengths = sum(int((b - a).sum()) for a, b, _ in (tm.note_frame_ranges(*_arrays(c[0])) for c in cases))
    assert counts[:, 1].sum() < lengths
    # the words are the dense roll of the definition
    for p in (0, 7, 100):
        for s in (0, 1):
            want = F.dense_roll(cases[p][s], 62.5, 400)
            bits = (roll[p, s][:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
            assert (bits.reshape(128, -1)[:, :400].T.astype(bool) == want).all()
    # a shorter roll clips, and both forms count the same entries
    _, _, clipped, _ = _both(packed, 62.5, 100)
    assert clipped.sum() > 100


def _arrays(notes):
    return (np.asarray([(s, e) for s, e, _ in notes], np.float64).reshape(-1, 2), np.asarray([p for _, _, p in notes], np.float64))


@pytest.mark.parametrize("fps", [62.5, 100.0])
def test_boundary_cases_have_their_closed_forms(fps):
    cases, want = F.boundary_cases(TILE, fps)
    counts, skipped, clipped, _ = _both(F.pack(cases), fps, 5 * TILE + 3)
    assert counts.tolist() == [list(w) for w in want]
    assert skipped.sum(0).tolist() == [5, 4] and not clipped.any()
    # b beyond n_frames: clipped and counted, the frames up to n_frames kept
    counts, skipped, clipped, _ = _both(F.pack(cases), fps, 4 * TILE)
    at = [i for i, c in enumerate(cases) if c[0] and c[0][0][2] == 64][0]
    assert clipped[at].tolist() == [1, 0] and counts[at].tolist() == [3 * TILE, 3 * TILE + 7, 3 * TILE]
    assert clipped.sum() == 1


def test_index_outside_the_table_is_skipped():
    cases, _ = F.union_cases()
    packed = F.pack(cases)
    packed.ref_idx[0], packed.est_idx[0] = -1, len(packed.est_meta)
    counts, skipped, clipped, _ = _both(packed, 62.5, 200)
    assert skipped[0].tolist() == [1, 1] and skipped[1:].sum() == 0 and counts[0].tolist() == [0, 40, 0]


def test_unions():
    cases, want = F.union_cases()
    counts, _, _, _ = _both(F.pack(cases), 62.5, 200)
    assert counts.tolist() == [list(w) for w in want]
    from contrib import transcription_metrics as tm
    for (ref, est), c in zip(cases, counts.tolist()):
        assert tm.frame_counts(*_arrays(ref), *_arrays(est)) == tuple(c)
    assert tm.scores_from_counts(*counts[3]) == (0.0, 0.0, 0.0) and tm.frame_scores(*_arrays([]), *_arrays(cases[3][1])) == (0.0,) * 3
    assert tm.frame_scores(*_arrays(cases[1][0]), *_arrays(cases[1][1])) == (1.0, 1.0, 1.0)


def test_grid_times_follow_the_f64_product():
    found = F.disagreeing_grid_times()
    assert len(found) == 20
    cases = [([(k * 0.01, k * 0.01 + 0.1, 60)], [(k * 0.01, k * 0.01 + 0.1, 60)]) for k, _ in found]
    n_frames = int(found[-1][0] * 0.625) + 20
    counts, _, _, roll = _both(F.pack(cases), 62.5, n_frames)
    for (k, exact), words in zip(found, roll[:, 0, 60]):
        bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)
        first = int(np.flatnonzero(bits)[0])
        assert first == int(np.floor(np.float64(k * 0.01) * np.float64(62.5))) and first != exact, (k, first, exact)


def test_pianoroll_of_the_host_scorer():
    from contrib import transcription_metrics as tm
    notes = [(0.0, 0.1, 60), (0.05, 0.05, 61), (1.0, 0.5, 62), (0.3, 0.4, 128), (float("nan"), 1.0, 60)]
    roll = tm.pianoroll(*_arrays(notes))
    assert roll.shape == (63, 128) and (roll == F.dense_roll(notes, 62.5, 63)).all()
    assert roll[:, 60].sum() == 7 and roll[:, 61].sum() == 1 and roll[62, 62] and roll[:, 62].sum() == 1
    assert tm.pianoroll(*_arrays([])).shape == (0, 128)


def _new(d):
    return {k: v for k, v in d.items() if k.startswith("Frame") or "nstrument" in k}


def test_evaluate_host_path_with_frames_and_instruments():
    import evaluate
    ref, est = M.synthetic_midi(1)
    plain = evaluate.compute_transcription_metrics(ref, est)
    got = evaluate.compute_transcription_metrics(ref, est, frames=True, instruments=True)
    assert list(got) == list(plain) + list(evaluate.FRAME_KEYS + evaluate.INSTRUMENT_KEYS)
    assert {k: got[k] for k in plain} == plain
    assert 0 < got["Frame F1"] < 1 and got["Num instruments ref"] == 3      # programs 0, 1, 40; the drums are program 0
    for g in ("flat", "midi_class", "full"):
        plain = evaluate.mt3_program_aware_note_scores(ref, est, g)
        mine = evaluate.mt3_program_aware_note_scores(ref, est, g, frames=True, instruments=True)
        assert list(mine) == list(plain) + list(evaluate.FRAME_KEYS) + ["Frame F1 (%s)" % g] + list(evaluate.INSTRUMENT_KEYS)
        assert {k: mine[k] for k in plain} == plain
        assert mine["Frame F1"] == got["Frame F1"] and 0 < mine["Frame F1 (%s)" % g] < 1
        same = evaluate.mt3_program_aware_note_scores(ref, ref, g, frames=True, instruments=True)
        for k, v in _new(same).items():
            assert v == (3 if k.startswith("Num") else 1.0), (k, v)


def test_a_shifted_program_family_moves_the_program_aware_frame_score():
    import evaluate
    ref, _ = M.synthetic_midi(2)
    moved = M.midi([(i.program if i.is_drum else i.program + 8, i.is_drum, [(n.start, n.end, n.pitch) for n in i.notes])
                    for i in ref.instruments])
    same = evaluate.mt3_program_aware_note_scores(ref, ref, "full", frames=True, instruments=True)
    got = evaluate.mt3_program_aware_note_scores(ref, moved, "full", frames=True, instruments=True)
    assert got["Frame F1"] == same["Frame F1"] == 1.0
    assert got["Frame F1 (full)"] < same["Frame F1 (full)"] and got["Instrument F1"] < same["Instrument F1"]
    flat = evaluate.mt3_program_aware_note_scores(ref, moved, "flat", frames=True)
    assert flat["Frame F1 (flat)"] == 1.0            # pitched stays pitched


def test_instrument_scores():
    from contrib import transcription_metrics as tm
    assert tm.instrument_scores([0, 1, 40, 0], [0, 41]) == (3, 2, 0.5, 1 / 3, tm.f_measure(0.5, 1 / 3))
    assert tm.instrument_scores([], [1]) == (0, 1, 0.0, 0.0, 0.0) and tm.instrument_scores([2], []) == (1, 0, 0.0, 0.0, 0.0)
    assert tm.instrument_scores([5], [5]) == (1, 1, 1.0, 1.0, 1.0)


def test_argument_errors_are_value_errors():
    from mrmt3 import lib
    times, meta = torch.zeros(3, 2, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.int32)
    idx, first = torch.arange(3, dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32)
    good = dict(ref_times=times, ref_meta=meta, est_times=times, est_meta=meta, ref_idx=idx, ref_first=first, est_idx=idx,
                est_first=first, fps=62.5, n_frames=100)
    before = lib.note_frames_launches()
    for change in (dict(fps=0.0), dict(fps=-1.0), dict(fps=float("nan")), dict(fps=float("inf")), dict(n_frames=0),
                   dict(n_frames=(1 << 31) - 63), dict(n_frames=2.5), dict(ref_times=times.float()), dict(est_meta=meta[:, :3]),
                   dict(ref_idx=idx.long()), dict(est_first=first[:1]), dict(ref_first=first[:1], est_first=first[:1])):
        with pytest.raises(ValueError, match="note_frames"):
            lib.note_frames(**{**good, **change})
    with pytest.raises(RuntimeError):                # host tensors: no CPU fallback of the kernel
        lib.note_frames(**good)
    assert lib.note_frames_launches() == before


def test_library_version_and_symbols():
    from mrmt3 import lib
    so = lib.load()
    assert so.mrmt3_version() >= 128 and lib.MIN_VERSION >= 128
    for name in ("mrmt3_note_frames_workspace_bytes", "mrmt3_note_frames_fwd", "mrmt3_note_frames_launches"):
        assert name in lib._SIGS and hasattr(so, name)
    assert so.mrmt3_note_frames_workspace_bytes(10, 1000) == 0
    assert callable(lib.note_frames) and lib.FRAMES_MAX == (1 << 31) - 64
    # the C library refuses the same arguments before any launch (no device is touched)
    buf = (ctypes.c_longlong * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    args = dict(ref_times=p, ref_meta=p, n_ref=1, est_times=p, est_meta=p, n_est=1, ref_idx=p, ref_first=p, est_idx=p,
                est_first=p, n_prob=1, fps=62.5, n_frames=100, counts=p, skipped=p, clipped=p, roll=None, workspace=None,
                stream=None)
    before = lib.note_frames_launches()
    for change in (dict(ref_times=None), dict(counts=None), dict(clipped=None), dict(n_prob=0), dict(fps=0.0),
                   dict(fps=float("inf")), dict(fps=float("nan")), dict(n_frames=0), dict(n_frames=(1 << 31) - 63),
                   dict(n_ref=-1), dict(n_est=1 << 31), dict(ref_meta=ctypes.c_void_p(p.value + 8))):
        assert so.mrmt3_note_frames_fwd(*{**args, **change}.values()) == 1, change       # MRMT3_ERR_INVALID_ARG
        assert b"note_frames_fwd" in so.mrmt3_last_error()
    assert lib.note_frames_launches() == before


def test_frames_for():
    from mrmt3 import lib, scoring
    assert scoring.frames_for(0.0) == 1 and scoring.frames_for(-3.0) == 1 and scoring.frames_for(1.0) == 64
    assert scoring.frames_for(0.016) == 2 and scoring.frames_for(float("inf")) == lib.FRAMES_MAX
    assert scoring.frames_for(1e300) == lib.FRAMES_MAX
