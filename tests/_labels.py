"""Constructions the device-label tests share (tests/test_device_labels_cpu.py, tests/test_device_labels_gpu.py): the fuzz
tracks and rows of the row contract (include/mrmt3_hip.h: mrmt3_label_rows_fwd) and the DEFINITION a row is held to —
`Tokenizer.row_targets` of the tokenisation of the merged, speed-changed track, then `pad_targets`.  numpy only at import;
nothing here touches the library.
"""
import numpy as np

SUBSETS = ((0, 1, 2, 3), (0, 2), (1,), (2, 3))
SHIFTS = (0, 3, -5)
PROGRAMS = ((0, False), (0, True), (0, False), (40, False))      # two stems share a program, one is a drum stem


def fuzz_track(seed, grid, confined, name=None):
    """A 3-9 s track of 4 stems, 1-60 notes each, pitches 58-63 (same-key overlaps are common).  `grid`: times on a 5 ms
    grid (exact half steps, equal-time events), else drawn at random.  `confined`: every note inside the first 40 % of
    the audio, else notes run past its end."""
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.stems import StemTrack
    rs = np.random.RandomState(seed)
    seconds = float(rs.uniform(3.0, 9.0))
    limit = 0.4 * seconds if confined else seconds + 0.8
    audio, notes = [], []
    for s, (program, drum) in enumerate(PROGRAMS):
        audio.append(np.zeros(int(seconds * 16000) - 37 * s, np.float32))
        ns = NoteSequence()
        for _ in range(int(rs.randint(1, 61))):
            if grid:
                st = 0.005 * int(rs.randint(0, int(limit / 0.005)))
                en = st + 0.005 * int(rs.randint(1, 120))
            else:
                st = float(rs.uniform(0, limit))
                en = st + float(rs.uniform(0.003, 0.6))
            ns.notes.append(Note(st, en, int(rs.randint(58, 64)), 90, program, drum, 0))
        ns.total_time = max(n.end_time for n in ns.notes)
        notes.append(ns)
    return StemTrack(name or "fuzz%d_%d%d" % (seed, grid, confined), ["s%d" % s for s in range(4)], audio, notes,
                     list(PROGRAMS))


def collapse_track(shift=3):
    """Two stems of one program with one note each on the same pitch; stem 1's note starts one ulp BEFORE stem 0's, and the
    speed factor of `shift` rounds both starts to the same float64.  Unscaled, the group's order is (stem 1, stem 0);
    scaled, the starts tie and merged order decides: (stem 0, stem 1) — stem 0's note is cut to nothing, where the
    unscaled order would cut stem 1's.  Returns (track, row arrays of the one full-length row)."""
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.labels import tokenizer_frames
    from mrmt3.stems import StemTrack
    step, scale = speed(shift)
    # (scale is in (0.5, 1): from 1.5 on the products lie in [1, 2) like x, spaced closer than their ulp, so ties are common)
    x = next(v for v in (float(np.nextafter(1.5, 2.0)) + k * 2.0 ** -52 for k in range(4096))
             if v * scale == float(np.nextafter(v, 2.0)) * scale)
    hi = float(np.nextafter(x, 2.0))
    notes = [NoteSequence([Note(hi, hi + 0.3, 60, 90, 0, False, 0)], hi + 0.3),
             NoteSequence([Note(x, x + 0.2, 60, 90, 0, False, 0)], x + 0.2)]
    tr = StemTrack("collapse", ["a", "b"], [np.zeros(48000, np.float32)] * 2, notes, [(0, False), (0, False)])
    n = stretched_samples(tr, step)
    T = tokenizer_frames(n, 128)
    rows = dict(kept=[(0, 1)], start_frame=[0], n_frames=[T], total_frames=[T], scale=[scale], shift=[shift], n_samples=[n])
    return tr, rows


def fuzz_tracks(n_seeds):
    return [fuzz_track(100 * k + 2 * g + c, bool(g), bool(c)) for k in range(n_seeds) for g in (0, 1) for c in (0, 1)]


def speed(shift):
    """(step, scale) of a shift in semitones, as the batcher plans it."""
    from mrmt3.resample import ratio_step
    step = 1 << 32 if shift == 0 else ratio_step(2.0 ** (shift / 12.0))
    return step, float(1 << 32) / float(step)


def stretched_samples(track, step):
    from mrmt3.resample import out_length
    return max(n if step == 1 << 32 else out_length(n, step) for n in track.lengths())


def fuzz_rows(track, seed, hop=128):
    """Rows of one track as a dict of per-row arrays (what the kernel takes) plus `kept` and `n_samples` per row: every
    subset x shift x window at frame 0, the last 256 frames, a random 100-frame window, the last single frame."""
    from mrmt3.labels import tokenizer_frames
    rs = np.random.RandomState(seed)
    rows = {k: [] for k in ("kept", "start_frame", "n_frames", "total_frames", "scale", "shift", "n_samples")}
    for kept in SUBSETS:
        for shift in SHIFTS:
            step, scale = speed(shift)
            n = stretched_samples(track, step)
            T = tokenizer_frames(n, hop)
            r = int(rs.randint(0, T - 100))
            for f0, nf in ((0, min(256, T)), (max(0, T - 256), min(256, T)), (r, 100), (T - 1, 1)):
                for k, v in zip(rows, (kept, f0, nf, T, scale, shift, n)):
                    rows[k].append(v)
    return rows


def row_arrays(rows):
    """The kernel's per-row arguments of `fuzz_rows`' result: (keep uint64, start_frame, n_frames, total_frames int64,
    scale float64, shift int32)."""
    keep = np.array([sum(1 << s for s in kept) for kept in rows["kept"]], np.uint64)
    return (keep, np.array(rows["start_frame"], np.int64), np.array(rows["n_frames"], np.int64),
            np.array(rows["total_frames"], np.int64), np.array(rows["scale"], np.float64), np.array(rows["shift"], np.int32))


def definition_rows(tokenizer, track, rows, event_length=1024):
    """int64 [B, event_length]: every row by the definition.  One tokenisation per (subset, shift)."""
    from mrmt3.batching import pad_targets
    from mrmt3.stems import merged_note_sequence, speed_note_sequence
    feats, out = {}, []
    for kept, f0, nf, shift, n in zip(rows["kept"], rows["start_frame"], rows["n_frames"], rows["shift"], rows["n_samples"]):
        if (kept, shift) not in feats:
            ns = merged_note_sequence(track, kept)
            if shift != 0:
                ns = speed_note_sequence(ns, shift, speed(shift)[0])
            feats[(kept, shift)] = tokenizer.tokenize(ns, n)
        out.append(tokenizer.row_targets(feats[(kept, shift)], f0, nf))
    return pad_targets(out, event_length).numpy()
