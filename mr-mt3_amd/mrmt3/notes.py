"""Token rows -> notes: the arrays a decoded recording comes back as, the row contract of
`mrmt3_notes_decode_fwd` (include/mrmt3_hip.h) restated on the host, and the launch.

The notes of a recording are BY DEFINITION what `InferenceHandler._postprocess_batch` + `_to_event` +
`contrib.metrics_utils.event_predictions_to_ns` (or `_scored`) make of its token rows with `NoteEncodingWithTiesSpec` (or the
scored twin): the cut at the first EOS, `run_length_encoding.decode_events`, `note_sequences.decode_note_event`, the flush.
`decode_notes_host` computes that function on arrays, row by row, in numpy and plain Python: it is the oracle of the device
kernel and runs without a GPU; tests hold it to the definition.  `decode_notes` is the kernel: one launch for every segment
of every recording, no CPU fallback of the kernel itself — only a recording with more notes sounding at once than the
kernel's LDS holds (`status != 0`) is decoded on the host, and that recording alone.

`decode_notes_device` is `decode_notes` without the copy home: the notes of every recording stay on the device as one
`DeviceNotes`, what `mrmt3.scoring` scores.

The quirks of the definition are reproduced, not repaired: a row without EOS contributes no tokens, UNK cuts a row like EOS,
and the sounding notes come out in the insertion order of the host's dict.
"""
from __future__ import annotations

import dataclasses
import math
from typing import List, Optional

import numpy as np

from contrib import note_sequences, vocabularies
from mrmt3.grammar import EventGrammar

MIN_NOTE_DURATION = note_sequences.MIN_NOTE_DURATION
STATUS_CAPACITY = 1      # more notes sounded at once than the kernel holds (mrmt3.lib.NOTES_CAPACITY)


def check_codec(codec) -> None:
    """ValueError naming what differs if `codec` is not `contrib.vocabularies.build_codec`'s."""
    ranges = [(r.type, r.min_value, r.max_value) for r in codec._ranges[1:]]
    bins = vocabularies.num_velocity_bins_from_codec(codec)
    want = [("pitch", 0, 127), ("velocity", 0, bins), ("tie", 0, 0), ("program", 0, 127), ("drum", 0, 127)]
    if ranges != want:
        raise ValueError("device notes implement the codec of contrib.vocabularies.build_codec only (velocity bins: the "
                         "codec's own), this codec has the ranges %r" % (ranges,))
    if codec.steps_per_second != int(codec.steps_per_second) or codec.steps_per_second < 1:
        raise ValueError("device notes need a whole steps_per_second >= 1, the codec has %r" % (codec.steps_per_second,))


def velocity_table(codec) -> np.ndarray:
    """int32 [n_velocity]: the velocity of every velocity id (`vocabularies.bin_to_velocity`)."""
    bins = vocabularies.num_velocity_bins_from_codec(codec)
    return np.asarray([vocabularies.bin_to_velocity(b, bins) for b in range(bins + 1)], np.int32)


@dataclasses.dataclass
class NoteArrays:
    """One recording's notes in the host decoder's order.  times float64 [n, 2]: start and end; meta int32 [n, 4]: pitch,
    velocity, program | is_drum << 8, 0 (the field order of `mrmt3.labels.NoteTable`); logc float32 [n] or None: the value
    the host holds before `math.exp`, a note's confidence is exp(logc)."""
    times: np.ndarray
    meta: np.ndarray
    logc: Optional[np.ndarray]
    invalid: int
    dropped: int
    total_time: float
    status: int = 0

    def __len__(self) -> int:
        return len(self.meta)

    def to_note_sequence(self, min_confidence: Optional[float] = None) -> note_sequences.NoteSequence:
        """The `NoteSequence` of the host path: `flush_note_decoding_state`'s, or `..._scored`'s with `confidence` set and
        the notes below `min_confidence` dropped before the instruments are assigned."""
        if min_confidence is not None and self.logc is None:
            raise ValueError("min_confidence needs scored notes (decode with logp)")
        Note = note_sequences.Note
        times, meta = self.times.tolist(), self.meta.tolist()
        notes = [Note(t[0], t[1], m[0], m[1], m[2] & 0xff, bool(m[2] >> 8 & 1)) for t, m in zip(times, meta)]
        if self.logc is not None:
            for note, lc in zip(notes, self.logc.tolist()):
                note.confidence = math.exp(lc)
            if min_confidence is not None:
                notes = [n for n in notes if n.confidence >= min_confidence]
        ns = note_sequences.NoteSequence(notes, float(self.total_time))
        note_sequences.assign_instruments(ns)
        return ns


def segment_times(frame_times, codec, recordings=None):
    """(seg_first int32 [n_rec + 1], start_time f64 [rows], limit f64 [rows], order) of the rows whose frame times are
    `frame_times` [rows, frames] (only column 0 is read), exactly as `_to_event` and `decode_and_combine_predictions`
    derive them: a row starts at its first frame's time minus the remainder mod 1 / steps_per_second, a recording's rows are
    taken in the order of their start times (a stable sort: `order`, row indices, None when they are in order already), and a
    row's limit is the next row's start, 0.0 (none) for the last and for a next row that starts at 0.0 (`if max_time`).
    `recordings`: the row count of every recording, None for a single one."""
    first = [ft[0] for ft in frame_times]
    rows = len(first)
    counts = [rows] if recordings is None else [int(c) for c in recordings]
    if any(c < 0 for c in counts) or sum(counts) != rows:
        raise ValueError("recordings %r do not add up to the %d rows" % (counts, rows))
    step = 1 / codec.steps_per_second
    start = np.zeros(rows, np.float64)
    for i, t in enumerate(first):
        t = np.float64(t)
        start[i] = t - t % step
    if rows and not (start >= 0).all():
        raise ValueError("segment start times must be >= 0 (a limit <= 0 means none)")
    seg_first = np.zeros(len(counts) + 1, np.int32)
    seg_first[1:] = np.cumsum(counts)
    order = np.arange(rows)
    for a, b in zip(seg_first[:-1], seg_first[1:]):
        order[a:b] = a + np.argsort(start[a:b], kind="stable")
    start = start[order]
    limit = np.zeros(rows, np.float64)
    for a, b in zip(seg_first[:-1], seg_first[1:]):
        limit[a:b - 1] = start[a + 1:b]
    return seg_first, start, limit, (None if (order == np.arange(rows)).all() else order)


def check_seg_first(seg_first, rows: int) -> None:
    s = np.asarray(seg_first)
    if s.ndim != 1 or len(s) < 2 or s[0] != 0 or s[-1] != rows or (np.diff(s) < 0).any():
        raise ValueError("seg_first must be non-decreasing from 0 to rows = %d, got %r" % (rows, s.tolist()))


def _decode_recording(ids, logp, start_time, limit, g: EventGrammar, velocity_of_bin, sps) -> NoteArrays:
    """The row contract for the rows of ONE recording."""
    W = ids.shape[1] - 1
    ranges = ((g.shift0, g.n_shift, "shift"), (g.pitch0, g.n_pitch, "pitch"), (g.velocity0, g.n_velocity, "velocity"),
              (g.tie, 1, "tie"), (g.program0, g.n_program, "program"), (g.drum0, g.n_drum, "drum"))
    scored = logp is not None
    times, meta, logc = [], [], []
    total = 0.0
    active = {}                                  # (program, pitch) -> [onset, velocity, logc], in insertion order
    current_time, velocity, program = 0.0, note_sequences.DEFAULT_VELOCITY, 0
    invalid = dropped = 0

    def emit(start, end, pitch, vel, prog, drum, lc):
        nonlocal total
        least = start + MIN_NOTE_DURATION
        if least > end:
            end = least
        times.append((start, end))
        meta.append((pitch, vel, prog | drum << 8, 0))
        logc.append(lc)
        if end > total:
            total = end

    for r in range(len(ids)):
        row = ids[r, 1:].tolist()
        cut = [j for j, t in enumerate(row) if t == g.eos or t == g.shift0 - 1]
        n = cut[0] if cut else 0                 # no EOS: no tokens
        t0, lim = float(start_time[r]), float(limit[r])
        tied, tie_section = set(), True
        steps, now = 0, t0
        program_lp = shift_lp = None
        for j in range(n):
            tok = row[j]
            kind = None
            for lo, cnt, name in ranges:
                if lo <= tok < lo + cnt:
                    kind, value = name, tok - lo
                    break
            if kind is None:
                invalid += 1
                continue
            lp = float(logp[r, j + 1]) if scored else 0.0
            if kind == "shift":
                steps += value
                now = t0 + steps / sps
                if lim > 0 and now > lim:
                    dropped += n - j
                    break
                shift_lp = lp
                continue
            steps = 0
            if now < current_time:
                invalid += 1
                continue
            lc = lp
            for other in (program_lp, shift_lp):
                if other is not None and other < lc:
                    lc = other
            current_time = now
            if kind == "pitch":
                key = (program, value)
                if tie_section:
                    if key not in active or key in tied:
                        invalid += 1
                    else:
                        tied.add(key)
                elif velocity == 0:
                    if key not in active:
                        invalid += 1
                    else:
                        onset, vel, olc = active.pop(key)
                        emit(onset, now, value, vel, program, 0, olc)
                else:
                    if key in active:
                        onset, vel, olc = active.pop(key)
                        emit(onset, now, value, vel, program, 0, olc)
                    active[key] = (now, velocity, lc)
            elif kind == "drum":
                if velocity == 0:
                    invalid += 1
                else:
                    emit(now, now + note_sequences.DEFAULT_NOTE_DURATION, value, velocity, 0, 1, lc)
            elif kind == "velocity":
                velocity = int(velocity_of_bin[value])
            elif kind == "program":
                program = value
                program_lp = lp
            else:                                # tie
                if not tie_section:
                    invalid += 1
                else:
                    for key in [k for k in active if k not in tied]:
                        onset, vel, olc = active.pop(key)
                        emit(onset, current_time, key[1], vel, key[0], 0, olc)
                    tie_section = False
    for onset, _, _ in active.values():
        if onset + MIN_NOTE_DURATION > current_time:
            current_time = onset + MIN_NOTE_DURATION
    for key, (onset, vel, olc) in active.items():
        emit(onset, current_time, key[1], vel, key[0], 0, olc)
    return NoteArrays(np.asarray(times, np.float64).reshape(-1, 2), np.asarray(meta, np.int32).reshape(-1, 4),
                      np.asarray(logc, np.float32) if scored else None, invalid, dropped, total)


def decode_notes_host(grammar: EventGrammar, ids, seg_first, start_time, limit, velocity_of_bin, steps_per_second,
                      logp=None) -> List[NoteArrays]:
    """The contract of `mrmt3_notes_decode_fwd` on the host, the arguments of `lib.notes_decode` as numpy arrays: one
    `NoteArrays` per recording, `status` always 0 (the host has no capacity)."""
    ids = np.asarray(ids, np.int64)
    if ids.ndim != 2 or ids.shape[1] < 2:
        raise ValueError("ids must be [rows, ld >= 2], got shape %s" % (ids.shape,))
    check_seg_first(seg_first, len(ids))
    if steps_per_second != int(steps_per_second) or steps_per_second < 1:
        raise ValueError("steps_per_second must be a whole number >= 1, got %r" % (steps_per_second,))
    if grammar.n_pitch > 128 or grammar.n_program > 128:
        raise ValueError("n_pitch and n_program must be <= 128")
    if logp is not None:
        logp = np.asarray(logp, np.float32)
        assert logp.shape == ids.shape, (logp.shape, ids.shape)
    out = []
    for a, b in zip(seg_first[:-1], seg_first[1:]):
        out.append(_decode_recording(ids[a:b], None if logp is None else logp[a:b], start_time[a:b], limit[a:b], grammar,
                                     velocity_of_bin, int(steps_per_second)))
    return out


_TABLES = {}


def _decode_launch(ids_dev, frame_times, codec, logp, recordings, eos_token_id, pad_token_id):
    """The launch `decode_notes` and `decode_notes_device` share: the checks, the row order, ONE `lib.notes_decode`, the
    per-recording head read back, and the notes written gathered on the device (one copy of what is needed instead of the
    regions whole).  Returns a dict; `redo(r)` decodes recording r on the host (a recording over the kernel's capacity)."""
    import torch
    from mrmt3 import lib
    from mrmt3.scoring import _home
    check_codec(codec)
    if not ids_dev.is_cuda or (logp is not None and not logp.is_cuda):
        raise RuntimeError("decode_notes needs device tensors (no CPU fallback of the kernel): decode_notes_host is the host's")
    if ids_dev.dim() != 2 or ids_dev.shape[0] != len(frame_times):
        raise ValueError("ids must be [rows, ld] with one row per entry of frame_times, got %s and %d"
                         % (tuple(ids_dev.shape), len(frame_times)))
    rows, ld = ids_dev.shape
    dev = ids_dev.device
    seg_first, start, limit, order = segment_times(frame_times, codec, recordings)
    check_seg_first(seg_first, rows)
    ids_dev = ids_dev.to(torch.int64)
    if logp is not None:
        logp = logp.float()
    if order is not None:
        at = torch.from_numpy(order).to(dev)
        ids_dev = ids_dev[at]
        logp = None if logp is None else logp[at]
    ids_dev = ids_dev.contiguous()
    logp = None if logp is None else logp.contiguous()
    grammar = EventGrammar.from_codec(codec, eos_token_id=eos_token_id, pad_token_id=pad_token_id)
    key = (str(dev), grammar.n_velocity)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(velocity_table(codec)).to(dev)
    sps = int(codec.steps_per_second)
    scalars = torch.from_numpy(np.concatenate([start, limit])).to(dev)
    out = lib.notes_decode(grammar, ids_dev, torch.from_numpy(seg_first).to(dev), scalars[:rows], scalars[rows:], _TABLES[key],
                           sps, logp)
    n_rec = len(seg_first) - 1
    *head, total = _home(*(out[k] for k in ("n_notes", "invalid", "dropped", "status", "total_time")))
    counts = np.where(head[3] == 0, head[0], 0)
    pick = np.concatenate([int(seg_first[r]) * (ld - 1) + np.arange(counts[r]) for r in range(n_rec)] or [np.zeros(0, int)])
    at = torch.from_numpy(pick.astype(np.int64)).to(dev)

    def redo(r):
        a, b = int(seg_first[r]), int(seg_first[r + 1])
        arrays = decode_notes_host(grammar, ids_dev[a:b].cpu().numpy(), np.asarray([0, b - a]), start[a:b], limit[a:b],
                                   velocity_table(codec), sps, None if logp is None else logp[a:b].cpu().numpy())[0]
        arrays.status = int(head[3][r])
        return arrays

    return dict(n_rec=n_rec, head=head, total=total, counts=counts, redo=redo, times=out["times"][at], meta=out["meta"][at],
                logc=None if logp is None else out["logc"][at])


def _recordings(d, *tables):
    """The walk over a launch's recordings: per recording (r, slices, redo) with `slices` its rows of each of `tables`
    (laid end to end in recording order, as `_decode_launch` gathers them; None stays None) and `redo` None, or, for a
    recording over the kernel's capacity, its `NoteArrays` decoded on the host (`slices` is then empty)."""
    o = 0
    for r in range(d["n_rec"]):
        n = int(d["counts"][r])
        yield r, [None if t is None else t[o:o + n] for t in tables], d["redo"](r) if d["head"][3][r] != 0 else None
        o += n


def decode_notes(ids_dev, frame_times, codec, logp=None, recordings=None, eos_token_id=1, pad_token_id=0) -> List[NoteArrays]:
    """ids_dev [rows, ld] int64 on the device as the decoder returned them (every row of every recording, a recording's rows
    together), frame_times [rows, frames] on the host, `codec` of `vocabularies.build_codec`, logp [rows, ld] f32 on the
    device or None, `recordings` the row count of each recording (None: one) -> one `NoteArrays` per recording.  One launch;
    only the notes written come back.  A recording over the kernel's capacity is decoded by `decode_notes_host`."""
    d = _decode_launch(ids_dev, frame_times, codec, logp, recordings, eos_token_id, pad_token_id)
    head, total = d["head"], d["total"]
    host = [None if t is None else t.cpu().numpy() for t in (d["times"], d["meta"], d["logc"])]
    return [redo if redo is not None else NoteArrays(*mine, int(head[1][r]), int(head[2][r]), float(total[r]))
            for r, mine, redo in _recordings(d, *host)]


@dataclasses.dataclass
class DeviceNotes:
    """The notes of several recordings as tensors on one device, for `mrmt3.scoring`: times float64 [N, 2] and meta int32
    [N, 4] in the layout of `NoteArrays` / `mrmt3.labels.NoteTable`; recording r's notes are the rows
    [first[r], first[r] + count[r]) (int64 [R]); invalid, dropped, status int32 [R] and total_time float64 [R] as the decoder
    reported them (zeros for tables that were not decoded).  `counts` is the host's copy of `count`, kept so that nothing
    is read back to learn a size."""
    times: "torch.Tensor"
    meta: "torch.Tensor"
    first: "torch.Tensor"
    count: "torch.Tensor"
    invalid: "torch.Tensor"
    dropped: "torch.Tensor"
    total_time: "torch.Tensor"
    status: "torch.Tensor"
    counts: Optional[np.ndarray] = None

    def __len__(self) -> int:
        return int(self.count.numel())

    def host_counts(self) -> np.ndarray:
        if self.counts is None:
            self.counts = self.count.cpu().numpy().astype(np.int64)
        return self.counts

    def entries(self, recording=None):
        """(rec, rows): per entry the recording and the table row, int64 on the notes' device, recording after recording;
        `recording=r`: the entries of that recording alone."""
        import torch
        dev, R, total = self.meta.device, len(self), int(self.host_counts().sum())
        count = self.count.to(torch.int64)
        rec = torch.repeat_interleave(torch.arange(R, device=dev), count, output_size=total)
        begin = torch.cumsum(count, 0) - count
        rows = self.first.to(torch.int64)[rec] + (torch.arange(total, device=dev) - begin[rec])
        if recording is not None:
            keep = rec == int(recording)
            rec, rows = rec[keep], rows[keep]
        return rec, rows

    @classmethod
    def _undecoded(cls, times, meta, counts, total_time) -> "DeviceNotes":
        """Tables that were not decoded: `times` and `meta` on their device, `counts` the host's rows per recording, laid end
        to end; invalid, dropped and status are zeros, `total_time` a list of floats."""
        import torch
        dev, zeros = meta.device, lambda: torch.zeros(len(counts), dtype=torch.int32, device=meta.device)
        return cls(times, meta, torch.from_numpy(np.cumsum(counts) - counts).to(dev), torch.from_numpy(counts).to(dev), zeros(),
                   zeros(), torch.tensor(total_time, dtype=torch.float64, device=dev), zeros(), counts)

    @classmethod
    def from_arrays(cls, tables, device) -> "DeviceNotes":
        """`tables`: one (times [n, 2], meta [n, 4]) pair of numpy arrays (or a `NoteArrays`) per recording, uploaded."""
        import torch
        pairs = [(t.times, t.meta) if hasattr(t, "meta") else t for t in tables]
        counts = np.asarray([len(m) for _, m in pairs], np.int64)
        times = np.concatenate([np.asarray(t, np.float64).reshape(-1, 2) for t, _ in pairs] or [np.zeros((0, 2))])
        meta = np.concatenate([np.asarray(m, np.int32).reshape(-1, 4) for _, m in pairs] or [np.zeros((0, 4), np.int32)])
        return cls._undecoded(torch.from_numpy(times).to(device), torch.from_numpy(meta).to(device), counts,
                              [float(t.total_time) if hasattr(t, "total_time") else 0.0 for t in tables])

    @classmethod
    def from_note_table(cls, times, meta=None) -> "DeviceNotes":
        """One recording: a track's reference, `mrmt3.labels.NoteTable` tensors already on a device (`times`, `meta`, or an
        object that has both).  No copy."""
        if meta is None:
            times, meta = times.times, times.meta
        return cls._undecoded(times, meta, np.asarray([meta.shape[0]], np.int64), [0.0])

    @classmethod
    def concat(cls, parts) -> "DeviceNotes":
        """Several `DeviceNotes` of one device as one, the recordings in order."""
        import torch
        parts = list(parts)
        offs = np.cumsum([0] + [p.meta.shape[0] for p in parts])
        cat = lambda name: torch.cat([getattr(p, name) for p in parts])
        return cls(cat("times"), cat("meta"), torch.cat([p.first + int(o) for p, o in zip(parts, offs)]), cat("count"),
                   cat("invalid"), cat("dropped"), cat("total_time"), cat("status"),
                   np.concatenate([p.host_counts() for p in parts]))


def decode_notes_device(ids_dev, frame_times, codec, recordings=None, eos_token_id=1, pad_token_id=0) -> DeviceNotes:
    """`decode_notes` without the copy home: the same launch, the notes stay on the device as one `DeviceNotes` (unscored).
    Only the per-recording head comes back.  A recording with `status != 0` is decoded on the host and uploaded, that one
    alone."""
    import torch
    d = _decode_launch(ids_dev, frame_times, codec, None, recordings, eos_token_id, pad_token_id)
    head, counts, dev = d["head"], d["counts"].astype(np.int64), ids_dev.device
    times, meta, total = d["times"], d["meta"], d["total"].copy()
    invalid, dropped = head[1].copy(), head[2].copy()
    if (head[3] != 0).any():
        tparts, mparts = [], []
        for r, (t, m), redo in _recordings(d, times, meta):
            if redo is not None:
                t, m = torch.from_numpy(redo.times).to(dev), torch.from_numpy(redo.meta).to(dev)
                counts[r], invalid[r], dropped[r], total[r] = len(redo), redo.invalid, redo.dropped, redo.total_time
            tparts.append(t)
            mparts.append(m)
        times, meta = torch.cat(tparts), torch.cat(mparts)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)
    return DeviceNotes(times, meta, up(np.cumsum(counts) - counts, torch.int64), up(counts, torch.int64),
                       up(invalid, torch.int32), up(dropped, torch.int32), up(total, torch.float64),
                       up(head[3], torch.int32), counts)
