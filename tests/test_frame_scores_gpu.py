"""Frame counts and piano rolls on a real MI355X: mrmt3_note_frames_fwd against the contract's host restatement
(`mrmt3.scoring.frame_counts_host`, which tests/test_frame_scores_cpu.py holds to the interval form and to closed forms) over
the corpus, the boundary values and the unions of tests/_frame_cases.py; then `scoring.pianoroll`, `score_tables` with
frames and instruments, the path from token rows to frame scores, `train.validate_notes`, and the options switched off.
Counts, words and scores are compared with `==`."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _frame_cases as F  # noqa: E402
import _note_match as M  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                                       # 32-bit words on either side of every output array
SENTINEL = -0x5a5a5a5a
_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mr-mt3_amd", "csrc", "frames.hip")
TILE = int(re.search(r"#define NF_TILE (\d+)", open(_SOURCE).read()).group(1))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


def _guarded(words, dev):
    return torch.full((words + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int32)


def _inner(buf):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "a guard word was written"
    return host[GUARD:-GUARD]


def _launch(packed, dev, fps, n_frames, with_roll=True):
    """One launch through the C ABI, guard words around every output and around the (empty) workspace:
    (counts, skipped, clipped, roll or None) on the host."""
    from mrmt3 import lib
    so = lib.load()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = [up(a) for a in packed.arrays()]
    spare = torch.zeros(16, device=dev, dtype=torch.int32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else spare.data_ptr())
    n_prob, W = len(packed.ref_first) - 1, -(-n_frames // 32)
    words = so.mrmt3_note_frames_workspace_bytes(n_prob, n_frames) // 4
    outs = [_guarded(n, dev) for n in (6 * n_prob, 2 * n_prob, 2 * n_prob, n_prob * 2 * 128 * W if with_roll else 0, words)]
    inner = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * GUARD)
    before = lib.note_frames_launches()
    rc = so.mrmt3_note_frames_fwd(ptr(keep[0]), ptr(keep[1]), len(packed.ref_meta), ptr(keep[2]), ptr(keep[3]),
                                  len(packed.est_meta), ptr(keep[4]), ptr(keep[5]), ptr(keep[6]), ptr(keep[7]), n_prob, fps,
                                  n_frames, inner(outs[0]), inner(outs[1]), inner(outs[2]), inner(outs[3]) if with_roll else None,
                                  inner(outs[4]), None)
    assert rc == 0, so.mrmt3_last_error()
    torch.cuda.synchronize()
    assert lib.note_frames_launches() == before + 1
    counts, skipped, clipped, roll, _ = (_inner(o) for o in outs)
    return (counts.view(np.int64).reshape(n_prob, 3), skipped.reshape(n_prob, 2), clipped.reshape(n_prob, 2),
            roll.view(np.uint32).reshape(n_prob, 2, 128, W) if with_roll else None)


def _same(got, want):
    for name, a, b in zip(("counts", "skipped", "clipped", "roll"), got, want):
        if a is not None and b is not None:
            assert a.shape == b.shape and (a == b).all(), (name, np.argwhere(a != b)[:5])


def _oracle(packed, fps, n_frames):
    from mrmt3 import scoring
    return scoring.frame_counts_host(*packed.arrays(), fps, n_frames, with_roll=True)


def test_corpus_in_one_launch(dev):
    cases = F.corpus()
    packed = F.pack(cases)
    assert len(cases) >= 300
    want = _oracle(packed, 62.5, 400)
    assert want[0][:, 0].sum() > 10000
    got = _launch(packed, dev, 62.5, 400)
    _same(got, want)
    _same(_launch(packed, dev, 62.5, 400), got)                    # the same bits again
    _same(_launch(packed, dev, 62.5, 400, with_roll=False)[:3], want[:3])
    # a roll that is no whole number of words, and one that cuts notes
    for n_frames in (333, 97):
        want = _oracle(packed, 62.5, n_frames)
        _same(_launch(packed, dev, 62.5, n_frames), want)
    assert want[2].sum() > 100


@pytest.mark.parametrize("fps", [62.5, 100.0])
def test_boundary_values(dev, fps):
    cases, closed = F.boundary_cases(TILE, fps)
    packed = F.pack(cases)
    packed.ref_idx[packed.ref_first[4]] = -1                        # index -1 and index n: skipped and counted
    packed.est_idx[packed.est_first[4]] = len(packed.est_meta)
    for n_frames in (5 * TILE + 3, 4 * TILE, 3 * TILE + 1):         # the second and third cut the longest note
        want = _oracle(packed, fps, n_frames)
        got = _launch(packed, dev, fps, n_frames)
        _same(got, want)
        if n_frames > 4 * TILE + 9:
            assert not got[2].any() and got[1].sum(0).tolist() == [6, 5]
            for p, c in enumerate(closed):
                assert got[0][p].tolist() == (list(c) if p != 4 else [0, 0, 0]), p
        else:
            assert got[2].sum() >= 1
    # one frame, at the very end of a roll that ends inside a word of the last tile
    one = F.pack([([(F.start_at(TILE + 40, fps), F.end_at(TILE + 41, fps), 127)], [(F.start_at(TILE + 40, fps), 0.0, 127)])])
    got = _launch(one, dev, fps, TILE + 41)
    _same(got, _oracle(one, fps, TILE + 41))
    assert got[0].tolist() == [[1, 1, 1]] and got[3][0, 0, 127, -1] == 1 << 8


def test_grid_times_follow_the_f64_product(dev):
    """Twenty of the times k * 0.01 at which floor(k * 0.01 * 62.5) in f64 is not the floor of the exact quotient."""
    found = F.disagreeing_grid_times()
    assert len(found) == 20
    packed = F.pack([([(k * 0.01, k * 0.01 + 0.1, 60)], [(k * 0.01, k * 0.01, 60)]) for k, _ in found])
    n_frames = int(found[-1][0] * 0.625) + 20
    got = _launch(packed, dev, 62.5, n_frames)
    _same(got, _oracle(packed, 62.5, n_frames))
    assert not got[1].any() and not got[2].any() and (got[0][:, 0] == 1).all()
    for (k, exact), words in zip(found, got[3][:, 0, 60]):
        bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)
        assert int(np.flatnonzero(bits)[0]) != exact                # the product's frame, not the exact quotient's


def test_unions(dev):
    from contrib import transcription_metrics as tm
    cases, closed = F.union_cases()
    packed = F.pack(cases)
    got = _launch(packed, dev, 62.5, 200)
    _same(got, _oracle(packed, 62.5, 200))
    assert got[0].tolist() == [list(c) for c in closed]
    assert got[0][1, 0] == got[0][1, 1] == got[0][1, 2] and got[0][2, 0] == 0
    assert tm.scores_from_counts(*got[0][3].tolist()) == (0.0, 0.0, 0.0) and tm.scores_from_counts(*got[0][5].tolist())[2] == 0.0


def test_senseless_first_arrays(dev):
    """Decreasing, negative, beyond the list length: the launch ends, nothing is written outside, and the result is what
    the clamping of the contract gives."""
    cases = F.corpus()[:12]
    packed = F.pack(cases)
    packed.ref_first[3], packed.ref_first[5], packed.est_first[2], packed.est_first[7] = 1 << 30, -5, -(1 << 31), 3
    packed.est_first[9] = packed.est_first[-1] + 1000
    got = _launch(packed, dev, 62.5, 400)
    _same(got, _oracle(packed, 62.5, 400))
    everything = F.pack(cases[:3])
    everything.ref_times[:], everything.est_times[:, 1] = np.nan, np.inf
    got = _launch(everything, dev, 62.5, 400)
    assert not got[0].any() and not got[3].any()
    assert got[1].tolist() == [[len(c[0]), len(c[1])] for c in cases[:3]]


def _tables(seed, sizes, programs=((0, 0), (1, 0), (40, 0), (0, 1))):
    """One (times, meta) table per recording; pitches 0..127 and a few outside."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        start = rng.integers(0, 4000, n) * 0.01
        times = np.stack([start, start + rng.integers(0, 80, n) * 0.01], 1).reshape(-1, 2)
        meta = np.zeros((n, 4), np.int32)
        meta[:, 0] = rng.integers(-2, 130, n)
        meta[:, 1] = 90
        pick = rng.integers(0, len(programs), n)
        meta[:, 2] = [programs[i][0] | programs[i][1] << 8 for i in pick]
        out.append((times, meta))
    return out


def test_pianoroll(dev):
    from contrib import transcription_metrics as tm
    from mrmt3 import lib, notes, scoring
    tables = _tables(11, (300, 0, 150))
    device_notes = notes.DeviceNotes.from_arrays(tables, dev)
    lib.note_frames_launches(reset=True)
    rolls = scoring.pianoroll(device_notes)
    assert lib.note_frames_launches() == 1 and len(rolls) == 3
    for (times, meta), roll in zip(tables, rolls):
        want = tm.pianoroll(times, meta[:, 0])
        assert roll.is_cuda and roll.dtype == torch.bool and tuple(roll.shape) == want.shape
        assert (roll.cpu().numpy() == want).all()
    assert tuple(rolls[1].shape) == (0, 128) and rolls[0].shape[0] > TILE
    assert (scoring.pianoroll(device_notes, recording=2).cpu().numpy() == rolls[2].cpu().numpy()).all()
    assert tuple(scoring.pianoroll(device_notes, recording=1).shape) == (0, 128)
    lib.note_frames_launches(reset=True)
    by = scoring.pianoroll(device_notes, by="program")
    assert lib.note_frames_launches() == 1 and by[1] == {}
    for (times, meta), mine, whole in zip(tables, by, rolls):
        keys = sorted({(int(m) & 0xff, bool(m >> 8 & 1)) for m in meta[:, 2]})
        assert sorted(mine) == keys
        for key in keys:
            rows = meta[:, 2] == (key[0] | int(key[1]) << 8)
            want = tm.pianoroll(times[rows], meta[rows, 0], n_frames=whole.shape[0])
            assert (mine[key].cpu().numpy() == want).all(), key
    at_100 = scoring.pianoroll(device_notes, fps=100.0, recording=0)
    assert (at_100.cpu().numpy() == tm.pianoroll(tables[0][0], tables[0][1][:, 0], fps=100.0)).all()


def _expected(ref, est):
    import evaluate
    want = dict(evaluate.compute_transcription_metrics(ref, est, frames=True, instruments=True))
    for g in ("flat", "full", "midi_class"):
        got = evaluate.mt3_program_aware_note_scores(ref, est, g, frames=True, instruments=True)
        want["F1 by program (%s)" % g] = got["F1 by program"]
        want.update(got)
    return want


def _same_scores(mine, want):
    assert set(mine) == set(want), set(mine) ^ set(want)
    for k in want:
        if "overlap" not in k:
            assert mine[k] == want[k], (k, mine[k], want[k])


def test_score_tables_with_frames_and_instruments(dev):
    import evaluate
    from mrmt3 import lib, scoring
    pairs = [M.synthetic_midi(s) for s in (1, 2, 3)]
    ref = [scoring.table_from_midi(r) for r, _ in pairs]
    est = [scoring.table_from_midi(e) for _, e in pairs]
    lib.note_match_launches(reset=True)
    lib.note_frames_launches(reset=True)
    plain = scoring.score_tables(ref, est, device=dev)
    assert lib.note_frames_launches() == 0 and lib.note_match_launches(reset=True) == 1
    got = scoring.score_tables(ref, est, device=dev, frames=True, instruments=True)
    assert lib.note_frames_launches() == 1 and lib.note_match_launches() == 1
    for pair, mine, before in zip(pairs, got, plain):
        want = {k: v for k, v in _expected(*pair).items() if "overlap" not in k}
        _same_scores(mine, want)
        extra = set(evaluate.FRAME_KEYS + evaluate.INSTRUMENT_KEYS) | {"Frame F1 (%s)" % g for g in scoring.GRANULARITIES}
        assert set(mine) - set(before) == extra and {k: mine[k] for k in before} == before
        assert all(0 < mine[k] < 1 for k in mine if k.startswith("Frame"))
    # evaluate.py's own device path, and the reference against itself
    for g in ("flat", "midi_class", "full"):
        assert evaluate.mt3_program_aware_note_scores(*pairs[1], g, device=dev, frames=True, instruments=True) == (
            evaluate.mt3_program_aware_note_scores(*pairs[1], g, frames=True, instruments=True))
    mine = evaluate.compute_transcription_metrics(*pairs[0], device=dev, frames=True, instruments=True)
    want = evaluate.compute_transcription_metrics(*pairs[0], frames=True, instruments=True)
    assert list(mine) == list(want) and all(mine[k] == want[k] for k in want if "overlap" not in k)
    same = scoring.score_tables(ref, ref, device=dev, frames=True, instruments=True)
    for res in same:
        assert all(res[k] == 1.0 for k in res if k.startswith("Frame") or k in evaluate.INSTRUMENT_KEYS[2:])
    with pytest.raises(ValueError, match="full"):
        scoring.score_tables(ref, est, device=dev, families=("on", "flat"), instruments=True)


def test_tokens_to_frame_scores_without_leaving_the_device(dev):
    import _notes as N
    import _stem_mix as sm
    from mrmt3 import labels, lib, notes, scoring
    from mrmt3.grammar import EventGrammar
    from test_note_match_gpu import _as_midi, _token_rows, _track_midi
    tracks = sm.synthetic_tracks(2)
    rows = [_token_rows(t) for t in tracks]
    width = max(ids.shape[1] for ids, _ in rows)
    ids = np.concatenate([np.pad(i, ((0, 0), (0, width - i.shape[1])), constant_values=N.PAD) for i, _ in rows])
    frame_times = np.concatenate([ft for _, ft in rows])
    recordings = [len(i) for i, _ in rows]
    for counter in (lib.note_match_launches, lib.notes_launches, lib.note_frames_launches):
        counter(reset=True)
    est = notes.decode_notes_device(torch.from_numpy(ids).to(dev), frame_times, N.CODEC, recordings=recordings)
    tables = [labels.note_table(t) for t in tracks]
    ref = notes.DeviceNotes.from_arrays([(t.times, t.meta) for t in tables], dev)
    got = scoring.score_tables(ref, est, frames=True, instruments=True)
    assert lib.notes_launches() == 1 and lib.note_match_launches() == 1 and lib.note_frames_launches() == 1
    seg_first, start, limit, order = notes.segment_times(frame_times, N.CODEC, recordings)
    host = notes.decode_notes_host(EventGrammar.from_codec(N.CODEC), ids, seg_first, start, limit, notes.velocity_table(N.CODEC),
                                   N.CODEC.steps_per_second)
    for track, arrays, mine in zip(tracks, host, got):
        want = {k: v for k, v in _expected(_track_midi(track), _as_midi(arrays)).items() if "overlap" not in k}
        _same_scores(mine, want)
        assert mine["Frame F1"] > 0.8


def test_validate_notes_with_frames(dev):
    import _stem_mix as sm
    import train
    from mrmt3 import labels, lib, notes
    from test_note_match_gpu import _as_midi, _track_midi
    tracks = sm.synthetic_tracks(2)
    tables = [labels.note_table(t) for t in tracks]
    reference = notes.DeviceNotes.from_arrays([(t.times, t.meta) for t in tables], dev)
    lib.note_frames_launches(reset=True)
    plain = train.validate_notes(None, tracks, dev, estimates=reference)
    assert lib.note_frames_launches() == 0 and "frame_f1" not in plain
    perfect = train.validate_notes(None, tracks, dev, estimates=reference, frames=True)
    assert lib.note_frames_launches() == 1 and perfect["frame_f1"] == 2.0 and perfect["onset_f1"] == plain["onset_f1"]
    first = notes.DeviceNotes.from_arrays([(tables[0].times, tables[0].meta)], dev)
    assert train.validate_notes(None, tracks[:1], dev, estimates=first, frames=True)["frame_f1"] == 1.0
    rng = np.random.default_rng(3)
    worse = []
    for t in tables:
        keep = rng.random(len(t.meta)) < 0.7
        move = np.maximum(rng.integers(-6, 7, int(keep.sum())) * 0.01, -t.times[keep, 0])
        worse.append(notes.NoteArrays(t.times[keep] + move[:, None], t.meta[keep], None, 0, 0, 0.0))
    got = train.validate_notes(None, tracks, dev, estimates=notes.DeviceNotes.from_arrays(worse, dev), frames=True)
    want = [_expected(_track_midi(t), _as_midi(w)) for t, w in zip(tracks, worse)]
    assert got["frame_f1"] == want[0]["Frame F1"] + want[1]["Frame F1"] and 0 < got["frame_f1"] < 2
    assert got["onset_f1"] == want[0]["Onset F1"] + want[1]["Onset F1"]


def test_options_off_launch_nothing(dev):
    import evaluate
    from mrmt3 import lib, scoring
    lib.note_frames_launches(reset=True)
    pair = M.synthetic_midi(1)
    host = evaluate.compute_transcription_metrics(*pair)
    mine = evaluate.compute_transcription_metrics(*pair, device=dev)
    assert list(mine) == list(host) and not any(k.startswith("Frame") or "nstrument" in k for k in mine)
    got = scoring.score_tables([scoring.table_from_midi(pair[0])], [scoring.table_from_midi(pair[1])], device=dev)[0]
    assert not any(k.startswith("Frame") or "nstrument" in k for k in got)
    assert lib.note_frames_launches() == 0
