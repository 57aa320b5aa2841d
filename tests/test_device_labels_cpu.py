"""Device-built stem-mix labels, the part that needs no GPU: `mrmt3.labels.label_rows_host` — the row contract
of include/mrmt3_hip.h restated — against the DEFINITION (tokenise the merged, speed-changed track, cut the row),
`Tokenizer.row_targets_prev`, the options and refusals of batcher and train.py, the C ABI's refusals, the loader's
triples.  Every comparison is integer equality."""
import ctypes
import dataclasses

import numpy as np
import pytest

import _labels as L
import _stem_mix as sm


@pytest.fixture(scope="module")
def tok():
    from mrmt3.tokenizer import Tokenizer
    return Tokenizer()


def test_host_restatement_equals_the_definition_on_the_fuzz(tok):
    """>= 1000 rows: 4 stems (programs 0, drum, 0, 40), 5 ms grid and random times, notes confined to the first 40 % and
    running past the end, four subsets, shifts 0 / +3 / -5, windows at frame 0, the last 256 frames, a random 100-frame
    window and the last single frame.  The definition raises on none of them and no row is skipped."""
    from mrmt3 import labels
    codec = labels.label_codec(tok)
    rows_seen = 0
    for i, tr in enumerate(L.fuzz_tracks(6)):
        rows = L.fuzz_rows(tr, i)
        want = L.definition_rows(tok, tr, rows)
        got, status = labels.label_rows_host(labels.note_table(tr), *L.row_arrays(rows), codec)
        assert not status.any()
        bad = np.nonzero((want != got).any(axis=1))[0]
        assert len(bad) == 0, (tr.name, {k: v[bad[0]] for k, v in rows.items()}, want[bad[0]][:48], got[bad[0]][:48])
        rows_seen += len(want)
    assert rows_seen >= 1000


def test_host_restatement_quirk_empty_subset_truncation_and_chunked_shifts(tok):
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3 import labels
    from mrmt3.stems import StemTrack
    codec = labels.label_codec(tok)
    one = NoteSequence([Note(0.1, 0.5, 60, 90, 0, False, 0)], 0.5)
    late = NoteSequence([Note(0.2, 0.3, 62, 90, 5, False, 0), Note(2.8, 2.9, 62, 90, 5, False, 0)], 2.9)
    tr = StemTrack("t", ["a", "b", "c"], [np.zeros(16000 * 4, np.float32)] * 3, [one, late, NoteSequence()],
                   [(0, False), (5, False), (0, False)])
    tab = labels.note_table(tr)
    T = labels.tokenizer_frames(64000, 128)
    i64 = lambda *v: np.array(v, np.int64)
    run = lambda mask, f0, nf, c=codec, length=1024: labels.label_rows_host(
        tab, np.array([mask], np.uint64), i64(f0), i64(nf), i64(T), np.ones(1), np.zeros(1, np.int32), c, length)[0][0]
    p, v, pi, tie = codec.program_base + 3, codec.velocity_base + 3, codec.pitch_base + 3, codec.tie_token + 3
    # the quirk: behind its only note a row repeats the state before the last step's first event
    assert run(1, 200, 100).tolist()[:5] == [p, pi + 60, tie, 1, -100]
    rows = dict(kept=[(0,)], start_frame=[200], n_frames=[100], shift=[0], n_samples=[64000])
    assert (L.definition_rows(tok, tr, rows)[0] == run(1, 200, 100)).all()
    # a kept subset without notes: `tie` alone (the definition raises IndexError)
    assert run(4, 0, 256).tolist()[:3] == [tie, 1, -100]
    with pytest.raises(IndexError):
        L.definition_rows(tok, tr, dict(kept=[(2,)], start_frame=[0], n_frames=[256], shift=[0], n_samples=[64000]))
    # a 2.5 s gap with max_shift_steps 100: the time since the row start in chunks, largest first
    short = dataclasses.replace(codec, max_shift_steps=100)
    assert run(2, 0, T, short).tolist()[:16] == [tie, 20 + 3, p + 5, v + 1, pi + 62, 30 + 3, v, pi + 62, 100 + 3, 100 + 3,
                                                 80 + 3, v + 1, pi + 62, 100 + 3, 100 + 3, 90 + 3]
    # truncation: a row that exactly fills event_length gets no EOS, one token fewer gets it
    full = run(2, 0, T, short, 1024)
    n = int(np.nonzero(full == 1)[0][0])
    assert (run(2, 0, T, short, n) == full[:n]).all() and run(2, 0, T, short, n + 1)[n] == 1


def test_host_restatement_orders_a_group_by_scaled_starts(tok):
    """Two starts one ulp apart that the speed factor rounds together: the definition orders them by merged index, not by
    their unscaled times, and so does the restatement (the kernel reports such a row, STATUS_ORDER)."""
    from mrmt3 import labels
    tr, rows = L.collapse_track()
    tab = labels.note_table(tr)
    assert tab.meta[:, 3].tolist() == [-1, 0]                             # the links: stem 1's note, then stem 0's
    got = labels.label_rows_host(tab, *L.row_arrays(rows), labels.label_codec(tok))[0]
    assert (got == L.definition_rows(tok, tr, rows)).all()
    off = int(np.nonzero(got[0] == labels.label_codec(tok).velocity_base + 3)[0][0])
    assert got[0, off - 1] == round((tr.notes[1].notes[0].end_time * rows["scale"][0]) * 100) + 3     # stem 1's note survives


def test_note_table_links_and_refusals():
    from mrmt3 import labels
    tr = L.fuzz_track(3, True, False)
    tab = labels.note_table(tr)
    assert tab.times.dtype == np.float64 and tab.meta.dtype == np.int32 and tab.meta.shape == (len(tab.times), 4)
    assert tab.nbytes == len(tab.times) * 32 and tab.n_stems == 4
    stems = tab.meta[:, 2] >> 16
    assert (np.diff(stems) >= 0).all() and [int((stems == s).sum()) for s in range(4)] == [len(ns.notes) for ns in tr.notes]
    for i, j in enumerate(tab.meta[:, 3]):
        if j >= 0:                               # the same group, not earlier, and (start, index) ascending
            assert tab.meta[i, 0] == tab.meta[j, 0] and (tab.meta[i, 2] & 0x1ff) == (tab.meta[j, 2] & 0x1ff)
            assert (tab.times[i, 0], i) < (tab.times[j, 0], j)
    assert len(set(tab.meta[:, 3][tab.meta[:, 3] >= 0].tolist())) == int((tab.meta[:, 3] >= 0).sum())
    assert labels.keep_masks(np.array([[1, 0, 1, 1], [0, 0, 0, 1]], bool)).tolist() == [13, 8]
    with pytest.raises(ValueError, match="1 to 64 stems"):
        labels.note_table(dataclasses.replace(tr, notes=tr.notes * 17))
    tr.notes[0].notes[0].start_time = -0.5
    with pytest.raises(ValueError, match="finite and >= 0"):
        labels.note_table(tr)


def test_row_targets_prev_boundary_and_placeholder(tok):
    from mrmt3.stems import merged_note_sequence
    tr = sm.synthetic_tracks(1)[0]
    feats = tok.tokenize(merged_note_sequence(tr, (0, 1, 2)), tr.n_samples)
    M = 64
    placeholder = tok.row_targets_prev(feats, 100 + M, 100, M)            # offset = mel_length: not > 0
    assert placeholder.tolist() == [tok.tie_token] == [1131]              # [tie, shift 1]: the trailing shift is dropped
    assert tok.row_targets_prev(feats, 100, 100, M).tolist() == [1131]    # a deterministic row: offset 0
    real = tok.row_targets_prev(feats, 100 + M + 1, 100, M)               # offset mel_length + 1: a real window
    assert (real == tok.row_targets(feats, 101, M)).all() and len(real) > 1
    from mrmt3.batching import pad_targets
    assert pad_targets([placeholder], 8).tolist() == [[1134, 1] + [-100] * 6]


def test_batcher_refuses_the_tokenizer_options_the_kernel_does_not_implement():
    from contrib import event_codec, vocabularies
    from mrmt3.batching import StemMixBatcher
    from mrmt3.tokenizer import Tokenizer
    for kw, name in ((dict(include_ties=False), "include_ties"), (dict(onsets_only=True), "onsets_only"),
                     (dict(is_train=False), "is_train"), (dict(is_randomize_tokens=True), "is_randomize_tokens")):
        with pytest.raises(ValueError, match=name):
            StemMixBatcher("cpu", tokenizer=Tokenizer(**kw), device_labels=True)
        StemMixBatcher("cpu", tokenizer=Tokenizer(**kw))                  # the host path takes them as before
    odd = event_codec.Codec(1000, 100, [event_codec.EventRange("pitch", 21, 108), event_codec.EventRange("velocity", 0, 1),
                                        event_codec.EventRange("tie", 0, 0), event_codec.EventRange("program", 0, 127),
                                        event_codec.EventRange("drum", 0, 127)])
    with pytest.raises(ValueError, match="codec"):
        StemMixBatcher("cpu", tokenizer=Tokenizer(codec=odd), device_labels=True)
    b = StemMixBatcher("cpu", tokenizer=Tokenizer(num_velocity_bins=127), device_labels=True)     # the codec's own bins
    assert b._codec.num_velocity_bins == 127 and b._codec.tie_token == 1001 + 128 + 128
    assert vocabularies.velocity_to_bin(90, 127) == 90
    with pytest.raises(ValueError, match="with_prev=True needs device_labels=True"):
        StemMixBatcher("cpu", with_prev=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StemMixBatcher("cpu", device_labels=True).build(sm.synthetic_tracks(1)[0])


def test_the_entry_point_is_declared_bound_and_refuses_bad_arguments_without_a_device():
    from mrmt3 import lib
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert lib._SIGS["mrmt3_label_rows_fwd"] == (ci, [vp, vp, ci, ci] + [vp] * 6 + [ci] * 12 + [vp, vp, vp])
    assert lib._SIGS["mrmt3_label_launches"] == (ctypes.c_ulonglong, [ci])
    so = lib.load()
    assert so.mrmt3_version() >= 125 and lib.MIN_VERSION >= 125 and callable(lib.label_rows)
    assert "mrmt3_label_rows_fwd" in lib.header_symbols() and hasattr(ctypes.CDLL(lib.LIB_PATH), "mrmt3_label_rows_fwd")
    buf = (ctypes.c_double * 8)()
    a = (ctypes.addressof(buf) + 15) & ~15
    lib.label_launches(reset=True)
    names = ("note_times", "note_meta", "n_notes", "n_stems", "keep", "start_frame", "n_frames", "total_frames", "scale",
             "shift", "batch", "pitch_base", "velocity_base", "tie_token", "program_base", "drum_base", "max_shift_steps",
             "steps_per_second", "sample_rate", "hop", "event_length", "num_special_tokens", "targets", "status", "stream")
    good = [a, a, 5, 4, a, a, a, a, a, a, 3, 1001, 1129, 1131, 1132, 1260, 1000, 100, 16000, 128, 1024, 3, a, a, None]
    assert len(names) == len(good) == len(lib._SIGS["mrmt3_label_rows_fwd"][1])
    cases = [(n, None, b"null") for n in ("note_times", "note_meta", "keep", "start_frame", "n_frames", "total_frames",
                                          "scale", "shift", "targets", "status")]
    cases += [("n_stems", 0, b"n_stems"), ("n_stems", 65, b"n_stems"), ("n_notes", -1, b"null note table"),
              ("batch", 0, b"must be > 0"), ("event_length", 0, b"must be > 0"), ("max_shift_steps", 0, b"must be > 0"),
              ("steps_per_second", -100, b"must be > 0"), ("sample_rate", 0, b"sample_rate"), ("hop", 0, b"hop"),
              ("tie_token", -1, b"token bases"), ("num_special_tokens", -3, b"token bases"), ("note_meta", a + 4, b"aligned")]
    for name, val, word in cases:
        args = list(good)
        args[names.index(name)] = val
        assert so.mrmt3_label_rows_fwd(*args) == 1 and word in so.mrmt3_last_error(), (name, val, so.mrmt3_last_error())
    assert lib.label_launches() == 0                                     # nothing was launched


def test_train_py_validates_stem_device_labels_and_lifts_the_with_prev_refusal(tmp_path):
    from mrmt3 import hydra_lite
    from test_config_cpu import MODEL, TOP
    import train
    (tmp_path / "model").mkdir()
    (tmp_path / "dataset").mkdir()
    (tmp_path / "config.yaml").write_text(TOP)
    (tmp_path / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    comp = lambda *over: hydra_lite.compose(str(tmp_path), "config", list(over))
    base = dict(root="/d", val_root=None, keep=0.75, gain_db=6.0, min_stems=1)
    assert train.stem_options(comp("+stem_root=/d")) == base              # the key appears only when given
    assert train.stem_options(comp("+stem_root=/d", "+stem_device_labels=true")) == dict(base, device_labels=True)
    assert train.stem_options(comp("+stem_root=/d", "+stem_device_labels=false")) == dict(base, device_labels=False)
    assert train.stem_options(comp("+stem_root=/d", "+stem_device_labels=true"), with_prev=True)["device_labels"] is True
    for over in ("+stem_device_labels=2", "+stem_device_labels=maybe"):
        with pytest.raises(ValueError, match="stem_device_labels"):
            train.stem_options(comp("+stem_root=/d", over))
    for over in ((), ("+stem_device_labels=false",)):
        with pytest.raises(ValueError, match="targets_prev, which the \\*WithPrev models train on, is not built"):
            train.stem_options(comp("+stem_root=/d", *over), with_prev=True)
    assert train.stem_options(comp("+stem_device_labels=true"), with_prev=True) is None


def test_stem_loader_yields_triples_when_the_batcher_builds_them():
    import torch
    import train

    class Stub:
        rng = None

        def build(self, track):
            return torch.full((2, 4, 8), float(track)), torch.full((2, 6), track), torch.full((2, 6), -track)

    batches = list(train.StemLoader([1, 2, 3, 4], Stub(), 2, seed=0, shuffle=False))
    assert len(batches) == 2 and all(len(b) == 3 for b in batches)
    mel, tg, prev = batches[1]
    assert mel.shape == (4, 4, 8) and tg[:, 0].tolist() == [3, 3, 4, 4] and prev[:, 0].tolist() == [-3, -3, -4, -4]
    got = list(train.loader_batches(batches, "cpu", 1, None))
    assert len(got) == 2 and got[0][3] is not None and (got[1][3] == prev).all()
