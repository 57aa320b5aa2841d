"""Constructions the cross-track tests share (tests/test_cross_mix_cpu.py, tests/test_cross_mix_gpu.py): tracks whose
(program, is_drum) pairs are disjoint from part to part, fuzz rows of 1-4 parts, the per-(row, part) arrays of
`mrmt3_label_rows_parts_fwd` (include/mrmt3_hip.h) and the DEFINITION a row is held to — `Tokenizer.row_targets` of the
tokenisation of `mrmt3.stems.virtual_note_sequence`, then `pad_targets`.  numpy only at import; nothing here touches the
library.
"""
import dataclasses

import numpy as np

import _labels as L

HOP = 128
DELAYS = (0, 1, 7, 250, 613)


def part_track(seed, grid, confined, p):
    """`_labels.fuzz_track` for part position p: position 0 keeps the fuzz programs (two stems on program 0, a drum stem,
    program 40); position p > 0 plays programs 10p, 10p + 5, 10p, 40 + p and has no drum stem, so no (program, is_drum)
    pair appears at two positions."""
    tr = L.fuzz_track(seed, grid, confined, name="part%d_%d_%d%d" % (p, seed, grid, confined))
    if p == 0:
        return tr
    programs = [(10 * p, False), (10 * p + 5, False), (10 * p, False), (40 + p, False)]
    for ns, (program, drum) in zip(tr.notes, programs):
        ns.notes = [dataclasses.replace(n, program=program, is_drum=drum) for n in ns.notes]
    return dataclasses.replace(tr, programs=programs)


def part_tracks(seed):
    """Four tracks, one per part position: both time grids, notes confined and running past the end."""
    return [part_track(10 * seed + p, bool((seed + p) & 1), bool((seed + p) >> 1 & 1), p) for p in range(4)]


@dataclasses.dataclass
class Row:
    parts: list                  # mrmt3.stems.VirtualPart, part 0 first
    start_frame: int             # F, in the virtual track's frames
    n_frames: int
    total_frames: int
    n_samples: int               # of the virtual track


def make_parts(tracks, kept, shifts, delays):
    from mrmt3.stems import VirtualPart
    return [VirtualPart(t, tuple(k), int(s), L.speed(int(s))[0], int(d)) for t, k, s, d in zip(tracks, kept, shifts, delays)]


def windows(parts, rs):
    """Rows of one part list: at frame 0, the virtual track's last 256 frames, a random 100-frame window, the last frame."""
    from mrmt3.labels import tokenizer_frames
    from mrmt3.stems import virtual_n_samples
    n = virtual_n_samples(parts, 16000, HOP)
    T = tokenizer_frames(n, HOP)
    r = int(rs.randint(0, T - 100))
    return [Row(parts, f0, nf, T, n) for f0, nf in ((0, min(256, T)), (max(0, T - 256), min(256, T)), (r, 100), (T - 1, 1))]


def fuzz_rows(tracks, seed, n_lists):
    """4 * n_lists rows over `part_tracks`: 1-4 parts (positions 0..n-1), every part a subset of `_labels.SUBSETS` (now and
    then none: an empty part), a shift of `_labels.SHIFTS` and a delay of DELAYS each; one part of every list has delay 0,
    as a planned row has."""
    rs = np.random.RandomState(seed)
    rows = []
    for k in range(n_lists):
        n_parts = 1 + k % 4
        kept = [L.SUBSETS[rs.randint(len(L.SUBSETS))] if rs.randint(12) else () for _ in range(n_parts)]
        shifts = [L.SHIFTS[rs.randint(3)] for _ in range(n_parts)]
        delays = [DELAYS[rs.randint(len(DELAYS))] for _ in range(n_parts)]
        delays[rs.randint(n_parts)] = 0
        rows += windows(make_parts(tracks[:n_parts], kept, shifts, delays), rs)
    return rows


def arena_of(tracks):
    """(arena NoteTable, {track name: (first note, note count)})."""
    from mrmt3 import labels
    tables = [labels.note_table(t) for t in tracks]
    arena, first = labels.note_arena(tables)
    return arena, {t.name: (int(f), len(tab.meta)) for t, f, tab in zip(tracks, first, tables)}


def row_arrays(rows, where, n_parts=None):
    """The per-(row, part) and per-row arguments of the entry, in its order after the arena: (note_first, note_count int32,
    keep uint64, delay_frames int64, scale float64, shift int32 [B, P]; start_frame, n_frames, total_frames int64 [B]).
    A row with fewer than P parts has empty ones behind (note_count 0, keep 0)."""
    P = n_parts or max(len(r.parts) for r in rows)
    B = len(rows)
    first, count, shift = (np.zeros((B, P), np.int32) for _ in range(3))
    keep, delay, scale = np.zeros((B, P), np.uint64), np.zeros((B, P), np.int64), np.ones((B, P), np.float64)
    for b, r in enumerate(rows):
        for p, part in enumerate(r.parts):
            first[b, p], count[b, p] = where[part.track.name]
            keep[b, p] = sum(1 << s for s in part.kept)
            delay[b, p], shift[b, p] = part.delay_frames, part.shift
            scale[b, p] = float(1 << 32) / float(part.step)
    return (first, count, keep, delay, scale, shift, np.array([r.start_frame for r in rows], np.int64),
            np.array([r.n_frames for r in rows], np.int64), np.array([r.total_frames for r in rows], np.int64))


def definition_rows(tokenizer, rows, event_length=1024):
    """int64 [B, event_length]: every row by the definition; one tokenisation per part list.  A virtual track without a
    single note is `tie` alone (the tokenizer raises IndexError there)."""
    from mrmt3.batching import pad_targets
    from mrmt3.stems import virtual_note_sequence
    feats, out = {}, []
    for r in rows:
        if id(r.parts) not in feats:
            ns = virtual_note_sequence(r.parts, 16000, HOP)
            feats[id(r.parts)] = tokenizer.tokenize(ns, r.n_samples) if ns.notes else None
        f = feats[id(r.parts)]
        out.append(np.array([tokenizer.tie_token]) if f is None else tokenizer.row_targets(f, r.start_frame, r.n_frames))
    return pad_targets(out, event_length).numpy()
