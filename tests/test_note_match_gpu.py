"""Note matching on a real MI355X: mrmt3_note_match_fwd against the contract's host restatement
(`mrmt3.scoring.match_notes_host`, which tests/test_note_match_cpu.py holds to the dense matcher and to scipy) over the
corpus, the boundary values and the chains of tests/_note_match.py; then `score_tables`, the path from token rows to
scores, `train.validate_notes`, and the options switched off.  Sizes and scores are compared with `==`."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _note_match as M  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                                       # 32-bit words on either side of every output array
SENTINEL = -0x5a5a5a5a


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables():
    from mrmt3 import scoring
    return scoring.pitch_tables()


def _guarded(words, dev):
    return torch.full((words + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int32)


def _inner(buf):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "a guard word was written"
    return host[GUARD:-GUARD]


def _launch(packed, tables, dev, onset_tol=0.05):
    """One launch through the C ABI, guard words around every output and around the workspace:
    (matched, match, status) on the host."""
    from mrmt3 import lib
    so = lib.load()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = [up(a) for a in packed.arrays()] + [up(t) for t in tables]
    spare = torch.zeros(16, device=dev, dtype=torch.int32)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else spare.data_ptr())
    n_prob, Lr, Le = len(packed.flags), len(packed.ref_idx), len(packed.est_idx)
    words = so.mrmt3_note_match_workspace_bytes(Lr, Le) // 4
    assert words == 4 * Le + 2 * Lr
    outs = [_guarded(n, dev) for n in (n_prob, Le, n_prob, words)]
    inner = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * GUARD)
    before = lib.note_match_launches()
    rc = so.mrmt3_note_match_fwd(ptr(keep[0]), ptr(keep[1]), len(packed.ref_meta), ptr(keep[2]), ptr(keep[3]),
                                 len(packed.est_meta), ptr(keep[4]), ptr(keep[5]), ptr(keep[6]), ptr(keep[7]), ptr(keep[8]),
                                 n_prob, ptr(keep[9]), ptr(keep[10]), len(tables[0]), onset_tol, 0.2, 0.05, inner(outs[0]),
                                 inner(outs[1]), inner(outs[2]), inner(outs[3]), None)
    assert rc == 0, so.mrmt3_last_error()
    torch.cuda.synchronize()
    assert lib.note_match_launches() == before + 1
    matched, match, status, _ = (_inner(o) for o in outs)
    return matched, match, status


def test_corpus_in_one_launch(dev, tables):
    from mrmt3 import scoring
    cases = M.corpus()
    packed = M.pack(cases)
    assert len(cases) >= 300 and any(len(c.ref_meta) == 0 for c in cases) and any(len(c.est_meta) == 0 for c in cases)
    want, _, _ = scoring.match_notes_host(*packed.arrays(), *tables)
    matched, match, status = _launch(packed, tables, dev)
    assert not status.any()
    assert (matched == want).all(), np.flatnonzero(matched != want)
    M.check_matching(packed, cases, matched, match)
    again = _launch(packed, tables, dev)
    assert (again[0] == matched).all() and (again[1] == match).all() and (again[2] == status).all()


def test_boundary_values(dev, tables):
    cases = M.boundary_cases()
    matched, match, status = _launch(M.pack(cases), tables, dev)
    assert not status.any()
    assert matched.tolist() == [int(M.dense_hit(c)[0, 0]) for c in cases]
    assert matched[:500].all() and matched[500:].tolist() == [1] * 8 + [0] * 4 + [1] * 4 + [0] * 4
    assert (match == np.where(matched == 1, np.arange(len(cases)), -1)).all()


def test_chains(dev, tables):
    """Past a wave, past a workgroup's threads, past any LDS: in one of the variants the search walks the whole chain."""
    built = [M.chain(n, first, last, mirror) for n in (65, 257, 1025) for mirror in (False, True) for first in (False, True)
             for last in (False, True)]
    cases = [b[0] for b in built]
    packed = M.pack(cases)
    # the closed forms stand on this adjacency: e_i next to r_{i-1} and r_i and to nothing else
    hit = M.dense_hit(cases[3])
    assert hit.sum() == 2 * 65 and all(hit[i, i] and hit[i + 1, i] for i in range(65))
    matched, match, status = _launch(packed, tables, dev, onset_tol=M.CHAIN_TOL)
    assert not status.any()
    assert matched.tolist() == [size for _, size, _ in built]
    M.check_matching(packed, cases, matched, match)
    for p, (case, _, unique) in enumerate(built):
        if unique is None:
            continue
        e0, e1 = packed.est_first[p], packed.est_first[p + 1]
        est = packed.est_idx[e0:e1] - packed.est_at[p]
        ref = packed.ref_idx[match[e0:e1]] - packed.ref_at[p]
        assert (ref == np.asarray([unique[int(i)] for i in est])).all(), p


def test_unordered_lists_and_edge_less_entries(dev, tables):
    from mrmt3 import scoring
    case, other = M.corpus()[5], M.corpus()[8]
    n = len(case.est_meta)
    packed = M.pack([other, case, case, other])
    e0 = packed.est_first[1]
    packed.est_idx[[e0, e0 + n - 1]] = packed.est_idx[[e0 + n - 1, e0]]               # problem 1's estimates out of order
    r0 = packed.ref_first[2]
    packed.ref_idx[[r0, r0 + 1]] = packed.ref_idx[[r0 + 1, r0]]
    assert packed.ref_times[packed.ref_idx[r0], 0] != packed.ref_times[packed.ref_idx[r0 + 1], 0]
    want = scoring.match_notes_host(*packed.arrays(), *tables)
    assert want[2].tolist() == [0, 2, 2, 0]
    matched, match, status = _launch(packed, tables, dev)
    assert status.tolist() == [0, 2, 2, 0] and matched.tolist() == want[0].tolist() and matched[0] > 0
    M.check_matching(M.pack([other]), [other], matched[:1], match[:packed.est_first[1]])
    assert (match[packed.est_first[1]:packed.est_first[3]] == -1).all()
    # indices outside the table, NaN onsets and offsets: no edges, the order undisturbed, and the launch ends
    packed = M.pack([case, other])
    packed.est_idx[1] = len(packed.est_meta) + 7
    packed.ref_idx[0] = -3
    packed.ref_times[packed.ref_idx[1], 0] = np.nan
    packed.est_times[packed.est_idx[packed.est_first[1]], 1] = np.nan
    want = scoring.match_notes_host(*packed.arrays(), *tables)
    matched, match, status = _launch(packed, tables, dev)
    assert status.tolist() == [0, 0] and matched.tolist() == want[0].tolist()
    assert match[1] == -1 and not np.isin(match, [0, 1]).any()
    assert (match >= 0).sum() == matched.sum()
    # `first` arrays that make no sense are clamped: nothing is written outside the outputs (the guards) and it ends
    packed = M.pack([case, other, case])
    packed.ref_first[1], packed.est_first[2] = 1 << 30, -5
    _launch(packed, tables, dev)
    everything = M.pack([case])
    everything.ref_times[:], everything.est_times[:] = np.nan, np.nan
    matched, match, status = _launch(everything, tables, dev)
    assert matched.tolist() == [0] and (match == -1).all()


def test_hostile_first_arrays_give_the_hosts_clamp(dev, tables):
    """`first` entries below 0, above the list length and decreasing: the ranges are those of the contract's clamp
    (csrc/notetab.h: note_range; `scoring._clamped`), no two problems share an entry, and matched, match and status are the
    host's with ==.  Three problems, at most 8 entries a list."""
    from mrmt3 import scoring
    cases = [M.chain(3, True, True, False)[0], M.chain(4, False, True, False)[0], M.chain(3, True, False, True)[0]]
    packed = M.pack(cases)
    (_, r1, _, Lr), (_, _, e2, Le) = packed.ref_first.tolist(), packed.est_first.tolist()
    packed.ref_first[:] = [-3, r1, Lr + 100, Lr]             # [0, r1), [r1, Lr), nothing
    packed.est_first[:] = [Le + 50, -5, e2, Le]              # nothing, [0, e2), [e2, Le)
    for idx, times, (a, b) in ((packed.ref_idx, packed.ref_times, (r1, Lr)), (packed.est_idx, packed.est_times, (0, e2))):
        part = idx[a:b].copy()                               # the lists of two cases as one, in onset order
        idx[a:b] = part[np.lexsort((part, times[part, 0]))]
    assert max(Lr - r1, e2) <= 8
    want = scoring.match_notes_host(*packed.arrays(), *tables, onset_tol=M.CHAIN_TOL)
    assert want[2].tolist() == [0, 0, 0] and want[0].tolist()[0] == want[0].tolist()[2] == 0 and want[0][1] >= 4
    got = _launch(packed, tables, dev, onset_tol=M.CHAIN_TOL)
    for name, a, b in zip(("matched", "match", "status"), got, want):
        assert (a == b).all(), (name, a.tolist(), b.tolist())


def _midi_pairs():
    return [M.synthetic_midi(s) for s in (1, 2, 3)]


def _expected(ref, est):
    import evaluate
    want = dict(evaluate.compute_transcription_metrics(ref, est))
    for g in ("flat", "full", "midi_class"):
        got = evaluate.mt3_program_aware_note_scores(ref, est, g)
        want["F1 by program (%s)" % g] = got["F1 by program"]
        want.update(got)
    return want


def _same_scores(mine, want, overlap=None):
    assert set(mine) == set(want), set(mine) ^ set(want)
    for k in want:
        if "overlap" in k:
            assert overlap is not None and mine[k] == overlap[k], (k, mine[k], overlap[k])
        else:
            assert mine[k] == want[k], (k, mine[k], want[k])


def test_score_tables_reproduces_evaluate(dev):
    from contrib import transcription_metrics as tm
    from mrmt3 import lib, scoring
    pairs = _midi_pairs()
    ref = [scoring.table_from_midi(r) for r, _ in pairs]
    est = [scoring.table_from_midi(e) for _, e in pairs]
    lib.note_match_launches(reset=True)
    got, matchings = scoring.score_tables(ref, est, with_overlap=True, device=dev, return_matching=True)
    assert lib.note_match_launches() == 1
    for r, (pair, mine) in enumerate(zip(pairs, got)):
        overlap = {f + "_overlap": tm.average_overlap_ratio(ref[r].times, est[r].times, matchings[r][f]) for f in ("onoff", "on")}
        for f in ("onoff", "on"):                # the matching returned is one: edges of the host's graph, each note once
            rows = matchings[r][f]
            assert len({a for a, _ in rows}) == len({b for _, b in rows}) == len(rows) == round(
                mine[f + "_precision"] * mine["len_est_intervals"])
        _same_scores(mine, _expected(*pair), overlap)
        assert 0 < mine["onoff_overlap"] <= 1
    plain = scoring.score_tables(ref, est, device=dev)
    assert lib.note_match_launches() == 2
    for mine, full in zip(plain, got):
        assert mine == {k: v for k, v in full.items() if "overlap" not in k}


def test_evaluate_functions_on_the_device(dev, tmp_path, capsys):
    import evaluate
    from contrib import midi_io, note_sequences
    from mrmt3 import lib
    pairs = _midi_pairs()
    want = evaluate.compute_transcription_metrics(*pairs[0])
    lib.note_match_launches(reset=True)
    got = evaluate.compute_transcription_metrics(*pairs[0], device=dev)
    assert list(got) == list(want)
    assert {k: v for k, v in got.items() if "overlap" not in k} == {k: v for k, v in want.items() if "overlap" not in k}
    assert 0 < got["on_overlap"] <= 1 and 0 < got["onoff_overlap"] <= 1     # (of the kernel's matching, not the host's)
    for g in ("flat", "midi_class", "full"):
        assert evaluate.mt3_program_aware_note_scores(*pairs[1], g, device=dev) == evaluate.mt3_program_aware_note_scores(
            *pairs[1], g)
    assert lib.note_match_launches(reset=True) == 4
    # evaluate_main: files on disk, every pair in one launch, the same keys and means
    for k, (ref, est) in enumerate(pairs):
        for mid, path in ((ref, tmp_path / "gt" / f"t{k}.mid"), (est, tmp_path / "out" / f"t{k}_16k.mid")):
            os.makedirs(path.parent, exist_ok=True)
            ns = midi_io.midi_to_note_sequence(mid)
            note_sequences.assign_instruments(ns)
            midi_io.note_sequence_to_midi_file(ns, str(path))
    host = evaluate.evaluate_main("ComMU", str(tmp_path / "out"), str(tmp_path / "gt"), enable_instrument_eval=True)
    assert lib.note_match_launches() == 0        # the option off: the host matcher, no launch
    mine = evaluate.evaluate_main("ComMU", str(tmp_path / "out"), str(tmp_path / "gt"), enable_instrument_eval=True, device=dev)
    assert lib.note_match_launches(reset=True) == 1
    assert list(mine) == list(host)
    for k in host:
        if k == "F1 by program":
            assert list(mine[k]) == list(host[k])
            assert all(abs(mine[k][p] - host[k][p]) < 1e-12 for p in host[k])
        else:                                    # (the host takes its means in the order its threads finish)
            assert abs(mine[k] - host[k]) < 1e-12, k
    capsys.readouterr()


# ---- from token rows and from audio ---------------------------------------------------------------------------------------
def _token_rows(track):
    """The track's notes as the decoder would return them: the tokenizer's rows of 256 frames, start token in front, EOS
    behind, padded; and the rows' frame times."""
    import _notes as N
    from mrmt3 import stems
    from mrmt3.tokenizer import Tokenizer
    tok = Tokenizer()
    ns = stems.merged_note_sequence(track, list(range(len(track.notes))))
    feats = tok.tokenize(ns, track.n_samples)
    frames = len(feats["input_times"])
    rows = [[int(t) + N.SP for t in tok.row_targets(feats, at, min(256, frames - at))] + [N.EOS] for at in range(0, frames, 256)]
    ids = np.full((len(rows), max(len(r) for r in rows) + 1), N.PAD, np.int64)
    for i, r in enumerate(rows):
        ids[i, 1:1 + len(r)] = r
    return ids, feats["input_times"][::256][:, None]


def _as_midi(arrays):
    """Decoded notes as the MIDI data `evaluate.py` reads: one instrument per (program, is_drum) in order of appearance."""
    from contrib import midi_io
    insts = {}
    for (start, end), m in zip(arrays.times.tolist(), arrays.meta.tolist()):
        key = (m[2] & 0xff, bool(m[2] >> 8 & 1))
        insts.setdefault(key, midi_io.MidiInstrument(key[0], key[1], [])).notes.append(midi_io.MidiNote(start, end, m[0], m[1]))
    return midi_io.MidiData(list(insts.values()), 220, 0.0)


def _track_midi(track):
    from mrmt3 import labels, notes
    table = labels.note_table(track)
    return _as_midi(notes.NoteArrays(table.times, table.meta, None, 0, 0, 0.0))


def test_tokens_to_scores_without_leaving_the_device(dev):
    import _notes as N
    import _stem_mix as sm
    from mrmt3 import labels, lib, notes, scoring
    from mrmt3.grammar import EventGrammar
    tracks = sm.synthetic_tracks(2)
    rows = [_token_rows(t) for t in tracks]
    width = max(ids.shape[1] for ids, _ in rows)
    ids = np.concatenate([np.pad(i, ((0, 0), (0, width - i.shape[1])), constant_values=N.PAD) for i, _ in rows])
    frame_times = np.concatenate([ft for _, ft in rows])
    recordings = [len(i) for i, _ in rows]
    lib.note_match_launches(reset=True)
    lib.notes_launches(reset=True)
    est = notes.decode_notes_device(torch.from_numpy(ids).to(dev), frame_times, N.CODEC, recordings=recordings)
    tables = [labels.note_table(t) for t in tracks]
    ref = notes.DeviceNotes.from_arrays([(t.times, t.meta) for t in tables], dev)
    got = scoring.score_tables(ref, est)
    assert lib.notes_launches() == 1 and lib.note_match_launches() == 1
    assert est.times.is_cuda and est.status.tolist() == [0, 0] and est.host_counts().sum() > 100
    # the host path on the same rows
    seg_first, start, limit, order = notes.segment_times(frame_times, N.CODEC, recordings)
    assert order is None
    host = notes.decode_notes_host(EventGrammar.from_codec(N.CODEC), ids, seg_first, start, limit, notes.velocity_table(N.CODEC),
                                   N.CODEC.steps_per_second)
    for track, arrays, mine in zip(tracks, host, got):
        want = {k: v for k, v in _expected(_track_midi(track), _as_midi(arrays)).items() if "overlap" not in k}
        _same_scores(mine, want)
        assert mine["Onset F1"] > 0.9 and mine["Onset + program F1 (full)"] > 0.9


def test_validate_notes(dev):
    import _stem_mix as sm
    import train
    from mrmt3 import labels, lib, notes
    from test_train_infer_gpu import _model
    tracks = sm.synthetic_tracks(2)
    tables = [labels.note_table(t) for t in tracks]
    reference = notes.DeviceNotes.from_arrays([(t.times, t.meta) for t in tables], dev)
    lib.note_match_launches(reset=True)
    perfect = train.validate_notes(None, tracks, dev, estimates=reference)
    assert perfect["tracks"] == 2 and perfect["onset_f1"] == 2.0 and perfect["onset_program_f1"] == 2.0
    assert lib.note_match_launches() == 1
    # an estimate with notes missing and moved, handed in: what the host scorer gives on the same notes
    rng = np.random.default_rng(3)
    worse = []
    for t in tables:
        keep = rng.random(len(t.meta)) < 0.7
        move = np.maximum(rng.integers(-6, 7, int(keep.sum())) * 0.01, -t.times[keep, 0])       # (no start before 0)
        worse.append(notes.NoteArrays(t.times[keep] + move[:, None], t.meta[keep], None, 0, 0, 0.0))
    got = train.validate_notes(None, tracks, dev, estimates=notes.DeviceNotes.from_arrays(worse, dev))
    want = [_expected(_track_midi(t), _as_midi(w)) for t, w in zip(tracks, worse)]
    assert got["onset_f1"] == want[0]["Onset F1"] + want[1]["Onset F1"] and 0 < got["onset_f1"] < 2
    assert got["onset_program_f1"] == want[0]["Onset + program F1 (flat)"] + want[1]["Onset + program F1 (flat)"]
    # through the model: its own inference path with device notes, the same numbers as the host scorer on those notes
    from test_device_notes_gpu import _EndsRows
    m = _EndsRows(_model("t5", dev).eval(), 46)
    import inference
    handler = inference.InferenceHandler(model=m, device=dev)
    est = handler.inference_many([train.full_mix(t) for t in tracks], max_length=48, return_tables=True)
    assert isinstance(est, notes.DeviceNotes) and est.times.is_cuda and len(est) == 2
    seqs = handler.inference_many([train.full_mix(t) for t in tracks], max_length=48, device_notes=True)
    assert [len(s.notes) for s in seqs] == est.host_counts().tolist() and sum(est.host_counts()) > 0
    lib.note_match_launches(reset=True)
    got = train.validate_notes(m, tracks, dev, max_length=48)
    assert lib.note_match_launches() == 1 and got["tracks"] == 2
    arrays, o = [], 0
    times, meta = est.times.cpu().numpy(), est.meta.cpu().numpy()
    for n in est.host_counts():
        arrays.append(notes.NoteArrays(times[o:o + n], meta[o:o + n], None, 0, 0, 0.0))
        o += n
    want = [_expected(_track_midi(t), _as_midi(a)) for t, a in zip(tracks, arrays)]
    assert got["onset_f1"] == want[0]["Onset F1"] + want[1]["Onset F1"]
    assert got["onset_program_f1"] == want[0]["Onset + program F1 (flat)"] + want[1]["Onset + program F1 (flat)"]


def test_options_off_launch_nothing(dev):
    """`inference_many`, `decode_notes` and the host scorer as they were: the same results, and the matcher is not launched."""
    import _notes as N
    import evaluate
    import inference
    from mrmt3 import lib, notes
    from mrmt3.synthetic import synth_audio
    from test_device_notes_gpu import _EndsRows
    from test_train_infer_gpu import _model
    lib.note_match_launches(reset=True)
    m = _EndsRows(_model("t5", dev).eval(), 46)
    h = inference.InferenceHandler(model=m, device=dev)
    audio = [synth_audio(1, n_samples=3 * 32768, seed=9)[0], synth_audio(1, n_samples=2 * 32768 + 100, seed=4)[0]]
    host = h.inference_many(audio, max_length=48)
    on_device = h.inference_many(audio, max_length=48, device_notes=True)
    tables = h.inference_many(audio, max_length=48, return_tables=True)
    assert [s.notes for s in on_device] == [s.notes for s in host]
    o = 0
    for seq, n in zip(host, tables.host_counts()):
        assert tables.times[o:o + n].cpu().tolist() == [[x.start_time, x.end_time] for x in seq.notes]
        assert tables.meta[o:o + n, 0].cpu().tolist() == [x.pitch for x in seq.notes]
        o += n
    case = N.corpus()[7]
    up = lambda a: torch.from_numpy(a).to(dev)
    got = notes.decode_notes(up(case.ids), case.frames[:, None], N.CODEC)
    N.same_arrays(got[0], N.host_arrays(case, False), case.name)
    kept = notes.decode_notes_device(up(case.ids), case.frames[:, None], N.CODEC)
    assert kept.times.cpu().numpy().tobytes() == got[0].times.tobytes()
    assert kept.meta.cpu().numpy().tobytes() == got[0].meta.tobytes()
    assert (kept.invalid.item(), kept.dropped.item(), kept.total_time.item()) == (got[0].invalid, got[0].dropped,
                                                                                 got[0].total_time)
    pair = M.synthetic_midi(1)
    assert evaluate.compute_transcription_metrics(*pair)["on_f1"] > 0
    with pytest.raises(ValueError):
        h.inference_many(audio, max_length=48, return_tables=True, with_confidence=True)
    assert lib.note_match_launches() == 0
