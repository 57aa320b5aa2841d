"""Stem-mix labels built row by row: the note table of a track, the codec descriptor, and the row contract of
`mrmt3_label_rows_fwd` (include/mrmt3_hip.h) restated on the host.

A row's targets are BY DEFINITION `Tokenizer.row_targets` of the tokenisation of the whole (merged, speed-changed) track
(`mrmt3.stems`).  They are a function of the kept stems' notes, the row's frame window and the speed factor alone, and
`label_rows_host` computes that function directly: filter, trim, sort, walk — no token stream of the whole track.  It is
the oracle of the device kernel and runs without a GPU (numpy and plain Python); tests hold it to the definition.

Two differences from the definition, both documented in the header:
  - a kept subset without a single event gives `tie` alone (the definition raises IndexError there);
  - the tie section of a row that starts behind the subset's last event is the state before the last step's first event
    (`encode_and_index_events` stops advancing its state mark in the trailing loop): reproduced, not repaired.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from contrib import vocabularies

MAX_STEMS = 64
# `status` of a row the kernel did not build exactly: the batcher rebuilds such a row on the host
STATUS_EVENTS = 1        # more events in the window than the kernel's LDS holds (mrmt3.lib.LABEL_CAPACITY)
STATUS_TIES = 2          # more sounding notes at the row's start than it holds
STATUS_ORDER = 4         # scaling collapsed two start times so that the table's links no longer give the group's order
STATUS_RANGE = 8         # a (shifted) pitch or a program outside 0..127


@dataclasses.dataclass(frozen=True)
class LabelCodec:
    """What the row contract needs of the event codec and of the frames."""
    pitch_base: int
    velocity_base: int
    tie_token: int
    program_base: int
    drum_base: int
    max_shift_steps: int
    steps_per_second: int
    sample_rate: int
    hop: int
    num_velocity_bins: int
    num_special_tokens: int = vocabularies.NUM_SPECIAL_TOKENS

    @property
    def frames_per_second(self) -> float:
        return self.sample_rate / self.hop


def check_tokenizer(tokenizer) -> None:
    """ValueError naming the option if `tokenizer` is not the configuration the row contract implements."""
    for name, want in (("include_ties", True), ("onsets_only", False), ("is_train", True), ("is_randomize_tokens", False)):
        if bool(getattr(tokenizer, name)) != want:
            raise ValueError("device labels implement %s=%s only, the tokenizer has %s=%r"
                             % (name, want, name, getattr(tokenizer, name)))
    codec = tokenizer.codec
    ranges = [(r.type, r.min_value, r.max_value) for r in codec._ranges[1:]]
    bins = vocabularies.num_velocity_bins_from_codec(codec)
    want = [("pitch", 0, 127), ("velocity", 0, bins), ("tie", 0, 0), ("program", 0, 127), ("drum", 0, 127)]
    if ranges != want:
        raise ValueError("device labels implement the codec of contrib.vocabularies.build_codec only (velocity bins: the "
                         "codec's own), the tokenizer's codec has the ranges %r" % (ranges,))
    if codec.steps_per_second != int(codec.steps_per_second) or codec.steps_per_second < 1:
        raise ValueError("device labels need a whole steps_per_second >= 1, the codec has %r" % (codec.steps_per_second,))


def label_codec(tokenizer) -> LabelCodec:
    check_tokenizer(tokenizer)
    codec, cfg = tokenizer.codec, tokenizer.cfg
    if cfg.sample_rate != int(cfg.sample_rate) or cfg.sample_rate < 1:
        raise ValueError("device labels need a whole sample_rate >= 1, the spectrogram config has %r" % (cfg.sample_rate,))
    base = {t: codec.event_type_range(t)[0] for t in ("pitch", "velocity", "tie", "program", "drum")}
    return LabelCodec(base["pitch"], base["velocity"], base["tie"], base["program"], base["drum"],
                      int(codec.max_shift_steps), int(codec.steps_per_second), int(cfg.sample_rate),
                      int(cfg.hop_width), vocabularies.num_velocity_bins_from_codec(codec))


@dataclasses.dataclass
class NoteTable:
    """Every stem's notes in stem order.  times float64 [N, 2]: start and end exactly as loaded.  meta int32 [N, 4]:
    pitch, velocity bin, program | is_drum << 8 | stem << 16, and the index of the note's successor in its
    (pitch, program, is_drum) group ordered by (start, index) over ALL stems, -1 for the last: a row follows the links to
    the first note of a kept stem."""
    times: np.ndarray
    meta: np.ndarray
    n_stems: int

    @property
    def nbytes(self) -> int:
        return self.times.nbytes + self.meta.nbytes


def note_table(track, num_velocity_bins: int = 1) -> NoteTable:
    if not 1 <= len(track.notes) <= MAX_STEMS:
        raise ValueError("a note table holds 1 to %d stems, the track has %d" % (MAX_STEMS, len(track.notes)))
    rows, times = [], []
    for s, ns in enumerate(track.notes):
        for n in ns.notes:
            if not (0.0 <= n.start_time < math.inf and 0.0 <= n.end_time < math.inf):
                raise ValueError("stem %d: note times must be finite and >= 0, got %r .. %r" % (s, n.start_time, n.end_time))
            if not (0 <= n.pitch <= 127 and 0 <= n.program <= 127):
                raise ValueError("stem %d: pitch %r / program %r outside 0..127" % (s, n.pitch, n.program))
            times.append((float(n.start_time) + 0.0, float(n.end_time) + 0.0))          # (+ 0.0: a -0.0 becomes +0.0)
            rows.append([int(n.pitch), vocabularies.velocity_to_bin(int(n.velocity), num_velocity_bins),
                         int(n.program) | int(bool(n.is_drum)) << 8 | s << 16, -1])
    times = np.asarray(times, np.float64).reshape(-1, 2)
    meta = np.asarray(rows, np.int32).reshape(-1, 4)
    groups = {}
    for i in range(len(meta)):
        groups.setdefault((int(meta[i, 0]), int(meta[i, 2]) & 0x1ff), []).append(i)
    for g in groups.values():
        g.sort(key=lambda i: times[i, 0])                                             # stable: equal starts keep index order
        for a, b in zip(g, g[1:]):
            meta[a, 3] = b
    return NoteTable(times, meta, len(track.notes))


def keep_masks(keep) -> np.ndarray:
    """bool [B, S] -> uint64 [B], bit s = stem s is kept."""
    keep = np.asarray(keep, bool)
    if keep.ndim != 2 or not 1 <= keep.shape[1] <= MAX_STEMS:
        raise ValueError("keep must be [rows, 1..%d stems], got shape %s" % (MAX_STEMS, keep.shape))
    return (keep.astype(np.uint64) << np.arange(keep.shape[1], dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def tokenizer_frames(n_samples: int, hop: int) -> int:
    """The tokenizer's frame count (`Tokenizer.frame_times`): a full extra hop when the samples are aligned."""
    return (int(n_samples) + hop - int(n_samples) % hop) // hop


def first_step(frame: int, codec: LabelCodec) -> int:
    """s0(frame): the largest step s with s / steps_per_second <= frame / frames_per_second, both quotients in float64."""
    sps = codec.steps_per_second
    t = float(np.float64(int(frame)) / np.float64(codec.frames_per_second))
    s = int(math.floor(t * sps))
    while (s + 1) / sps <= t:
        s += 1
    while s / sps > t:
        s -= 1
    return s


def _kept_notes(table: NoteTable, mask: int, scale: float, shift: int, delay: float = 0.0, part: int = 0) -> list:
    """[start, end, pitch, vbin, program, is_drum, (part, table index)] of the notes the mask keeps, as the row sees them:
    times scaled when shift != 0, then delayed when delay != 0, one rounding each."""
    notes = []
    for i in range(len(table.meta)):
        pitch, vbin, packed, _ = (int(v) for v in table.meta[i])
        if not mask >> (packed >> 16 & 63) & 1:
            continue
        st, en, drum = float(table.times[i, 0]), float(table.times[i, 1]), bool(packed >> 8 & 1)
        if shift != 0:
            st, en = st * scale, en * scale
            pitch = pitch if drum else pitch + shift
        if delay != 0.0:
            st, en = st + delay, en + delay
        notes.append([st, en, pitch, vbin, packed & 0xff, drum, (part, i)])
    return notes


def _row_tokens(table: NoteTable, mask: int, start_frame: int, n_frames: int, total_frames: int, scale: float, shift: int,
                codec: LabelCodec) -> list:
    """The row contract, token ids before `pad_targets`."""
    return _tokens_of_notes(_kept_notes(table, mask, scale, shift), start_frame, n_frames, total_frames, codec)[0]


def _tokens_of_notes(notes: list, start_frame: int, n_frames: int, total_frames: int, codec: LabelCodec):
    """Trim, sort, walk over `_kept_notes` lists -> (token ids, events in the window, tie pairs)."""
    sps = codec.steps_per_second
    groups = {}
    for n in notes:
        groups.setdefault((n[2], n[4], n[5]), []).append(n)
    for g in groups.values():
        g.sort(key=lambda n: n[0])               # stable: equal starts keep merged order
        for a, b in zip(g, g[1:]):
            if a[1] > b[0]:
                a[1] = b[0]
    events = []                                  # (time, on, is_drum, program, pitch, merged index, vbin)
    for st, en, pitch, vbin, program, drum, i in notes:
        if not st < en:
            continue
        if not drum:
            events.append((en, 0, drum, program, pitch, i, 0))
        events.append((st, 1, drum, program, pitch, i, vbin))
    events.sort()
    if not events:
        return [codec.tie_token], 0, 0           # (the definition raises IndexError here)
    steps = [round(e[0] * sps) for e in events]  # half to even, like rint
    lo = first_step(start_frame, codec)
    hi = first_step(start_frame + n_frames, codec) if start_frame + n_frames < total_frames else None
    bound = min(lo, steps[-1])                   # the quirk: behind the last event the state mark stays at the last step
    state = {}
    for e, s in zip(events, steps):
        if s < bound and not e[2]:
            state[(e[3], e[4])] = e[1]
    out, cur_program, cur_velocity = [], None, None
    ties = sorted(k for k, on in state.items() if on)
    in_window = 0
    for program, pitch in ties:
        if program != cur_program:
            out.append(codec.program_base + program)
            cur_program = program
        out.append(codec.pitch_base + pitch)
    out.append(codec.tie_token)
    flushed = 0
    for e, s in zip(events, steps):
        if s < lo or (hi is not None and s >= hi):
            continue
        in_window += 1
        _, on, drum, program, pitch, _, vbin = e
        if s - lo > flushed:                     # every event emits its pitch or drum token: the shift comes first
            left = flushed = s - lo
            while left > 0:
                out.append(min(codec.max_shift_steps, left))
                left -= out[-1]
        if not drum and program != cur_program:
            out.append(codec.program_base + program)
            cur_program = program
        if vbin != cur_velocity:
            out.append(codec.velocity_base + vbin)
            cur_velocity = vbin
        out.append((codec.drum_base if drum else codec.pitch_base) + pitch)
    return out, in_window, len(ties)


def label_rows_host(table: NoteTable, keep, start_frame, n_frames, total_frames, scale, shift, codec: LabelCodec,
                    event_length: int = 1024):
    """The contract of `mrmt3_label_rows_fwd` on the host: (targets int64 [B, event_length] in `pad_targets` form,
    status int32 [B], always 0 here: the host has no capacity).  keep uint64 [B] masks (`keep_masks`); the other per-row
    arguments as the kernel takes them."""
    B = len(keep)
    out = np.full((B, event_length), -100, np.int64)
    for b in range(B):
        row = _row_tokens(table, int(keep[b]), int(start_frame[b]), int(n_frames[b]), int(total_frames[b]),
                          float(scale[b]), int(shift[b]), codec)[:event_length]
        out[b, :len(row)] = np.asarray(row, np.int64) + codec.num_special_tokens
        if len(row) < event_length:
            out[b, len(row)] = 1
    return out, np.zeros(B, np.int32)


# ---- rows of virtual tracks -----------------------------------------------------------------------------------

MAX_PARTS = 4            # parts of one cross-track row (LB_MAX_PARTS, an ABI constant)
STATUS_SHARED = 16       # two parts of the row hold kept notes of one (program, is_drum): the per-part trim does not serve
CAPACITY = 2048          # events of a row's window, and tie pairs, that the kernels hold (mrmt3.lib.LABEL_CAPACITY)


def note_arena(tables):
    """Note tables one after the other, as `mrmt3_label_rows_parts_fwd` takes them: (NoteTable of all notes — its `next`
    links count from each table's own first note, so they are the tables' own —, first note of every table)."""
    first = np.concatenate([[0], np.cumsum([len(t.meta) for t in tables])]).astype(np.int64)
    times = np.concatenate([t.times.reshape(-1, 2) for t in tables]) if tables else np.zeros((0, 2), np.float64)
    meta = np.concatenate([t.meta.reshape(-1, 4) for t in tables]) if tables else np.zeros((0, 4), np.int32)
    return NoteTable(np.ascontiguousarray(times), np.ascontiguousarray(meta), max([t.n_stems for t in tables] + [1])), first[:-1]


def _part_status(table: NoteTable, mask: int, scale: float, shift: int, delay: float) -> int:
    """STATUS_RANGE and STATUS_ORDER of one part, found the way the kernel finds them: along the table's links."""
    n, flags = len(table.meta), 0
    kept = lambda i: bool(mask >> (int(table.meta[i, 2]) >> 16 & 63) & 1)

    def start(i):
        t = float(table.times[i, 0])
        t = t * scale if shift != 0 else t
        return t + delay if delay != 0.0 else t

    for i in range(n):
        if not kept(i):
            continue
        pitch, vbin, packed, j = (int(v) for v in table.meta[i])
        pitch = pitch + shift if shift != 0 and not packed >> 8 & 1 else pitch
        if not (0 <= pitch <= 127 and 0 <= (packed & 0xff) <= 127 and 0 <= vbin <= 127):
            flags |= STATUS_RANGE
            continue
        hops = 0
        while hops < n and 0 <= j < n and not kept(j):
            j, hops = int(table.meta[j, 3]), hops + 1
        if (shift != 0 or delay != 0.0) and 0 <= j < n and kept(j):
            if start(j) < start(i) or (start(j) == start(i) and j < i):
                flags |= STATUS_ORDER
    return flags


def label_rows_parts_host(arena: NoteTable, note_first, note_count, keep, delay_frames, scale, shift, start_frame, n_frames,
                          total_frames, codec: LabelCodec, event_length: int = 1024):
    """The contract of `mrmt3_label_rows_parts_fwd` on the host: (targets int64 [B, event_length] in `pad_targets` form,
    status int32 [B], the kernel's status words).  `arena`: the tables one after the other (`note_arena`); note_first,
    note_count, keep (uint64), delay_frames, scale, shift [B, P]; start_frame, n_frames, total_frames [B].  The tokens are
    the definition's — the trim runs over the whole row — so a row with status 16 is still the row the batcher wants; the
    kernel's tokens equal them wherever the status is 0."""
    keep = np.asarray(keep)
    B, P = keep.shape
    if not 1 <= P <= MAX_PARTS:
        raise ValueError("a row has 1 to %d parts, got %d" % (MAX_PARTS, P))
    N = len(arena.meta)
    fps = np.float64(codec.frames_per_second)
    out = np.full((B, event_length), -100, np.int64)
    status = np.zeros(B, np.int32)
    for b in range(B):
        notes, owners, flags = [], {}, 0
        for p in range(P):
            first, count, mask = int(note_first[b][p]), int(note_count[b][p]), int(keep[b][p])
            if first < 0 or first > N:
                first, count = 0, 0
            count = max(0, min(count, N - first))
            if mask == 0 or count == 0:
                continue
            d = int(delay_frames[b][p])
            delay = float(np.float64(d) / fps) if d > 0 else 0.0
            table = NoteTable(arena.times[first:first + count], arena.meta[first:first + count], arena.n_stems)
            flags |= _part_status(table, mask, float(scale[b][p]), int(shift[b][p]), delay)
            part = _kept_notes(table, mask, float(scale[b][p]), int(shift[b][p]), delay, p)
            for n in part:
                if owners.setdefault((n[4] & 0x7f, n[5]), p) != p:
                    flags |= STATUS_SHARED
            notes += part
        row, events, ties = _tokens_of_notes(notes, int(start_frame[b]), int(n_frames[b]), int(total_frames[b]), codec)
        flags |= (STATUS_EVENTS if events > CAPACITY else 0) | (STATUS_TIES if ties > CAPACITY else 0)
        row = row[:event_length]
        out[b, :len(row)] = np.asarray(row, np.int64) + codec.num_special_tokens
        if len(row) < event_length:
            out[b, len(row)] = 1
        status[b] = flags
    return out, status
