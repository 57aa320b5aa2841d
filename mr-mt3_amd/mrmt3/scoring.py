"""Note-level scores from device-resident note tables: the pitch tables, the problem lists and the host
restatement of `mrmt3_note_match_fwd` (include/mrmt3_hip.h), and `score_tables`, which reproduces `evaluate.py`'s numbers;
frame-level counts, piano rolls and instrument detection: the host restatement of `mrmt3_note_frames_fwd`,
`pianoroll`, and the `frames` / `instruments` options of `score_tables`.  Both paths go from entry keys to lists in `_lists`
and bring their small tensors home in `_home`.

The scores are BY DEFINITION those of `evaluate.compute_transcription_metrics` and `evaluate.mt3_program_aware_note_scores`
(the mir_eval restatement in `contrib.transcription_metrics`).  Precision, recall and F1 depend only on the SIZE of a maximum
matching, which is unique, so they are assembled from integers by the very expressions `evaluate.py` uses
(`tm.scores_from_counts`, `evaluate.program_aware_result`): the results are equal with `==`.  The overlap ratio depends on
WHICH maximum matching was found and may differ from the host's in the last digits, as the host's may from mir_eval's.

`match_notes_host` is the kernel's contract on numpy arrays: window-based, never an n x m matrix.  It is the oracle of the
kernel and runs without a GPU; tests hold it to `tm.match_notes`.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import List

import numpy as np

from contrib import transcription_metrics as tm

ONSET_TOLERANCE = 0.05
OFFSET_RATIO = 0.2
OFFSET_MIN_TOLERANCE = 0.05
PITCH_TOLERANCE = 50.0
STATUS_ORDER = 2         # a list of the problem is not in onset order
TABLE_MIDI_AS_HZ = 0     # compute_transcription_metrics and "Onset F1": MIDI numbers go to the matcher as if they were Hz
TABLE_HZ = 1             # the per-program scores: midi_to_hz values
FAMILIES = ("onoff", "on", "flat", "midi_class", "full")
GRANULARITIES = FAMILIES[2:]
MIN_PITCH, MAX_PITCH = 21, 108       # tm.sequence_to_valued_intervals


def pitch_tables():
    """(lo, hi) int32 [2, 128]: reference pitch r and estimated pitch e are within the pitch tolerance iff
    lo[t, r] <= e <= hi[t, r] (an empty range is lo > hi).  Each row comes from the expression of `tm.match_notes` on the
    128 values the matcher would be handed: table 0 the MIDI numbers themselves, table 1 `tm.midi_to_hz` of them.  Pitch 0 of
    table 0 has no edge (the host refuses a pitch <= 0)."""
    lo, hi = np.ones((2, 128), np.int32), np.zeros((2, 128), np.int32)
    midi = np.arange(128, dtype=np.float64)
    for t, values in ((TABLE_MIDI_AS_HZ, midi), (TABLE_HZ, tm.midi_to_hz(midi))):
        with np.errstate(divide="ignore", invalid="ignore"):
            cents = np.abs(1200.0 * np.subtract.outer(np.log2(values), np.log2(values)))
            hit = np.less_equal(cents, PITCH_TOLERANCE)
        if t == TABLE_MIDI_AS_HZ:
            hit[0, :] = hit[:, 0] = False
        for r in range(128):
            at = np.flatnonzero(hit[r])
            if len(at):
                assert (np.diff(at) == 1).all()              # (a pitch's neighbours are a range)
                lo[t, r], hi[t, r] = at[0], at[-1]
    return lo, hi


def _distance(a, b):
    return np.around(np.abs(a - b), decimals=tm.N_DECIMALS)


def _keys(times, idx):
    """(valid bool [L], key f64 [L]) of one list: an entry is valid when its index lies in the table and its onset is a
    number; the key is the onset of the nearest valid entry at or before it, -inf if there is none."""
    idx = np.asarray(idx, np.int64)
    n = len(times)
    valid = (idx >= 0) & (idx < n)
    onset = np.full(len(idx), np.nan)
    onset[valid] = times[idx[valid], 0]
    valid &= ~np.isnan(onset)
    last = np.maximum.accumulate(np.where(valid, np.arange(len(idx)), -1))
    key = np.where(last >= 0, onset[np.maximum(last, 0)], -np.inf)
    return valid, key


def _ordered(valid, key, idx) -> bool:
    at = np.flatnonzero(valid)
    k, i = key[at], np.asarray(idx, np.int64)[at]
    return bool(((k[:-1] < k[1:]) | ((k[:-1] == k[1:]) & (i[:-1] < i[1:]))).all())


def _clamped(first, p, L):
    """The list range of problem p as the kernels clamp it (csrc/notetab.h: note_range): a in [0, L], b in [a, L]."""
    a = min(max(int(first[p]), 0), L)
    return a, min(max(int(first[p + 1]), a), L)


def match_notes_host(ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first, prob_flags, pitch_lo,
                     pitch_hi, onset_tol=ONSET_TOLERANCE, offset_ratio=OFFSET_RATIO, offset_min_tol=OFFSET_MIN_TOLERANCE):
    """The contract of `mrmt3_note_match_fwd` on the host, the arguments of `lib.note_match` as numpy arrays ->
    (matched int32 [n_prob], match int32 [Le], status int32 [n_prob]).  The same decomposition as the kernel (order, exact
    windows, Kuhn's search from every estimated entry in list order, a free reference before a descent, the lowest
    first), so the matching itself is the kernel's, not only its size."""
    ref_times, est_times = np.asarray(ref_times, np.float64).reshape(-1, 2), np.asarray(est_times, np.float64).reshape(-1, 2)
    ref_pitch, est_pitch = np.asarray(ref_meta).reshape(-1, 4)[:, 0], np.asarray(est_meta).reshape(-1, 4)[:, 0]
    ref_idx, est_idx = np.asarray(ref_idx, np.int64), np.asarray(est_idx, np.int64)
    pitch_lo, pitch_hi = np.asarray(pitch_lo).reshape(-1, 128), np.asarray(pitch_hi).reshape(-1, 128)
    n_prob, Lr, Le = len(prob_flags), len(ref_idx), len(est_idx)
    assert len(ref_first) == n_prob + 1 and len(est_first) == n_prob + 1
    matched, status = np.zeros(n_prob, np.int32), np.zeros(n_prob, np.int32)
    match = np.full(Le, -1, np.int32)
    for p in range(n_prob):
        (r0, r1), (e0, e1) = _clamped(ref_first, p, Lr), _clamped(est_first, p, Le)
        offsets, table = bool(prob_flags[p] & 1), int(prob_flags[p]) >> 8
        r_valid, r_key = _keys(ref_times, ref_idx[r0:r1])
        e_valid, e_key = _keys(est_times, est_idx[e0:e1])
        if not (_ordered(r_valid, r_key, ref_idx[r0:r1]) and _ordered(e_valid, e_key, est_idx[e0:e1])):
            status[p] = STATUS_ORDER
            continue
        if not 0 <= table < len(pitch_lo):
            continue
        # the valid references' fields, by list position
        rn = np.where(r_valid, ref_idx[r0:r1], 0)
        r_on, r_off, r_pitch = ref_times[rn, 0], ref_times[rn, 1], ref_pitch[rn]
        r_ok = r_valid & (r_pitch >= 0) & (r_pitch < 128)
        r_lo, r_hi = pitch_lo[table][np.clip(r_pitch, 0, 127)], pitch_hi[table][np.clip(r_pitch, 0, 127)]
        with np.errstate(invalid="ignore"):
            r_tol = np.maximum(offset_ratio * (r_off - r_on), offset_min_tol)
        # windows: a coarse bracket by the keys, the exact predicate inside it
        margin = onset_tol + 1e-5
        wlo, whi = np.zeros(e1 - e0, np.int64), np.zeros(e1 - e0, np.int64)
        for k in range(e1 - e0):
            a = int(np.searchsorted(r_key, e_key[k] - margin, "left"))
            b = int(np.searchsorted(r_key, e_key[k] + margin, "right"))
            with np.errstate(invalid="ignore"):
                near = _distance(r_key[a:b], e_key[k]) <= onset_tol
            wlo[k] = a + int(np.count_nonzero(~((r_key[a:b] >= e_key[k]) | near)))
            whi[k] = b - int(np.count_nonzero((r_key[a:b] > e_key[k]) & ~near))
        owner = np.full(r1 - r0, -1, np.int64)
        stamp = np.zeros(r1 - r0, np.int64)

        def candidates(k):
            """(edge bool, free bool) over the window of estimated entry k"""
            a, b = wlo[k], whi[k]
            if not e_valid[k]:
                return np.zeros(b - a, bool), np.zeros(b - a, bool)
            en = est_idx[e0 + k]
            on_e, off_e, pitch_e = est_times[en, 0], est_times[en, 1], est_pitch[en]
            with np.errstate(invalid="ignore"):
                edge = r_ok[a:b] & (_distance(r_on[a:b], on_e) <= onset_tol)
                edge &= (r_lo[a:b] <= pitch_e) & (pitch_e <= r_hi[a:b])
                if offsets:
                    edge &= _distance(r_off[a:b], off_e) <= r_tol[a:b]
            return edge, owner[a:b] < 0

        for root in range(e1 - e0):
            cur, stack = root, []
            while True:
                edge, free = candidates(cur)
                a = wlo[cur]
                hit = np.flatnonzero(edge & free)
                if len(hit):
                    e, r = cur, a + int(hit[0])
                    while True:
                        owner[r] = e
                        match[e0 + e] = r0 + r
                        if not stack:
                            break
                        e, r = stack.pop()
                    matched[p] += 1
                    break
                down = np.flatnonzero(edge & ~free & (stamp[a:whi[cur]] != root + 1))
                if len(down):
                    r = a + int(down[0])
                    stamp[r] = root + 1
                    stack.append((cur, r))
                    cur = int(owner[r])
                elif stack:
                    cur = stack.pop()[0]
                else:
                    break
    return matched, match, status


# ---- frames ------------------------------------------------------------------------------------------------
FRAMES_PER_SECOND = tm.FRAMES_PER_SECOND
FRAME_LIMIT = 2147483648.0


def frame_counts_host(ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first, fps=FRAMES_PER_SECOND,
                      n_frames=1, with_roll=False):
    """The contract of `mrmt3_note_frames_fwd` on the host, the arguments of `lib.note_frames` as numpy arrays ->
    (counts int64 [n_prob, 3], skipped int32 [n_prob, 2], clipped int32 [n_prob, 2]) and, with `with_roll`, roll uint32
    [n_prob, 2, 128, W].  A dense bool roll per problem and side, packed into words at the end: the kernel's oracle."""
    tables = ((np.asarray(ref_times, np.float64).reshape(-1, 2), np.asarray(ref_meta).reshape(-1, 4)[:, 0],
               np.asarray(ref_idx, np.int64), ref_first),
              (np.asarray(est_times, np.float64).reshape(-1, 2), np.asarray(est_meta).reshape(-1, 4)[:, 0],
               np.asarray(est_idx, np.int64), est_first))
    n_prob, n_frames, fps = len(ref_first) - 1, int(n_frames), np.float64(fps)
    assert len(est_first) == n_prob + 1 and n_prob > 0 and n_frames >= 1 and np.isfinite(fps) and fps > 0
    W = -(-n_frames // 32)
    counts = np.zeros((n_prob, 3), np.int64)
    skipped, clipped = np.zeros((n_prob, 2), np.int32), np.zeros((n_prob, 2), np.int32)
    roll = np.zeros((n_prob, 2, 128, W), np.uint32) if with_roll else None
    for p in range(n_prob):
        dense = np.zeros((2, 128, W * 32), bool)
        for s, (times, pitches, idx, first) in enumerate(tables):
            L = max(int(first[n_prob]), 0)
            lo, hi = _clamped(first, p, L)
            for note in idx[lo:hi].tolist():
                if not 0 <= note < len(times):
                    skipped[p, s] += 1
                    continue
                start, end, pitch = times[note, 0], times[note, 1], int(pitches[note])
                with np.errstate(over="ignore", invalid="ignore"):
                    ps, pe = start * fps, end * fps
                if np.isnan(start) or np.isnan(end) or not 0 <= pitch <= 127 or not ps < FRAME_LIMIT or not pe < FRAME_LIMIT:
                    skipped[p, s] += 1
                    continue
                a = max(0, int(np.floor(max(ps, -1.0))))               # (max: -inf has no floor among the ints)
                b = max(a + 1, int(np.ceil(max(pe, -1.0))))
                if b > n_frames:
                    clipped[p, s] += 1
                dense[s, pitch, min(a, n_frames):min(b, n_frames)] = True
        counts[p] = (dense[0] & dense[1]).sum(), dense[0].sum(), dense[1].sum()
        if with_roll:
            roll[p] = np.packbits(dense, axis=-1, bitorder="little").reshape(2, 128, W, 4).view("<u4")[..., 0]
    return (counts, skipped, clipped, roll) if with_roll else (counts, skipped, clipped)


@dataclasses.dataclass
class MidiTable:
    """A MIDI file's notes as a table (instrument after instrument) and, for the program groups, every instrument's
    (program, is_drum) in order: an instrument without notes still names a group in `evaluate.py`."""
    times: np.ndarray
    meta: np.ndarray
    programs: list


def table_from_midi(mid) -> MidiTable:
    """`contrib.midi_io.MidiData` -> the note table `evaluate.py`'s scores are functions of."""
    times = [(n.start, n.end) for inst in mid.instruments for n in inst.notes]
    meta = [(n.pitch, n.velocity, int(inst.program) | int(bool(inst.is_drum)) << 8, 0)
            for inst in mid.instruments for n in inst.notes]
    return MidiTable(np.asarray(times, np.float64).reshape(-1, 2), np.asarray(meta, np.int32).reshape(-1, 4),
                     [(int(inst.program), bool(inst.is_drum)) for inst in mid.instruments])


@dataclasses.dataclass
class Problems:
    """What `build_problems` returns.  On the tables' device: ref_idx, ref_first, est_idx, est_first, prob_flags as
    `lib.note_match` takes them.  On the host, per problem: pair (the recording pair), family (an index into FAMILIES), key
    ((granular program, is_drum), None for the agnostic families), n_ref, n_est (the list lengths) and first_ref / first_est
    (the lowest table row on each side, the order of first appearance).  max_end: the largest end time of any note of
    either side (0.0 without notes; a NaN is passed over), what the length of the frame rolls is computed from."""
    ref_idx: "torch.Tensor"
    ref_first: "torch.Tensor"
    est_idx: "torch.Tensor"
    est_first: "torch.Tensor"
    prob_flags: "torch.Tensor"
    pair: np.ndarray
    family: np.ndarray
    key: list
    n_ref: np.ndarray
    n_est: np.ndarray
    first_ref: np.ndarray
    first_est: np.ndarray
    errors: list                                  # per pair: None, or the ValueError the host scorer would raise
    families: tuple = FAMILIES                    # the families built
    max_end: float = 0.0

    @functools.cached_property
    def by_pair(self) -> list:
        """Per recording pair {family: [its problems, ascending]}, built once."""
        index = [dict() for _ in self.errors]
        for p, (r, f) in enumerate(zip(self.pair, self.family)):
            index[int(r)].setdefault(int(f), []).append(p)
        return index


_NO_ROW = 1 << 40


def _home(*tensors):
    """Several small tensors of one device (int32, int64, f64) to the host in ONE copy: concatenated as int64 (an f64's
    bits ride as they are), copied, and cut up again -> one numpy array per tensor, with its dtype and shape."""
    import torch
    flat = [t.reshape(-1).view(torch.int64) if t.dtype == torch.float64 else t.reshape(-1).to(torch.int64) for t in tensors]
    data, out, o = torch.cat(flat).cpu().numpy(), [], 0
    for t in tensors:
        piece = data[o:o + t.numel()]
        piece = piece.view(np.float64) if t.dtype == torch.float64 else piece.astype(np.int32 if t.dtype == torch.int32 else np.int64)
        out.append(piece.reshape(tuple(t.shape)))
        o += t.numel()
    return out


def _lists(sides, forced):
    """Entry keys -> problems and their lists.  `sides`: per side (key, rows, pre, reduce): the int64 key and table row of
    every entry, `pre` None or a permutation of the entries that a problem's entries keep among themselves (None: the
    order they come in), `reduce` [(values, op, fill)], per-problem reductions of per-entry values; `forced`: keys that are
    a problem even without an entry.  -> (uniq, per side (n, idx int32, first int32, the reductions)): the sorted problem
    keys, and per side the list lengths, the lists end to end in problem order and where each begins."""
    import torch
    uniq = torch.unique(torch.cat([key for key, _, _, _ in sides] + [forced]))
    P, out = int(uniq.numel()), []
    for key, rows, pre, reduce in sides:
        pid = torch.searchsorted(uniq, key)
        order = torch.sort(pid, stable=True).indices if pre is None else pre[torch.sort(pid[pre], stable=True).indices]
        n = torch.bincount(pid, minlength=P)
        first = torch.cat([n.new_zeros(1), torch.cumsum(n, 0)]).to(torch.int32)
        reduced = [torch.full((P,), fill, dtype=torch.int64, device=key.device).scatter_reduce_(0, pid, values, op)
                   for values, op, fill in reduce]
        out.append((n, rows[order].to(torch.int32), first, reduced))
    return uniq, out


def _side(notes, families):
    """Per entry of one side: the table row, the recording, the problem key; and the [R, 4] validity counts."""
    import torch
    rec, rows = notes.entries()
    dev, R, total = notes.meta.device, len(notes), int(rows.numel())
    start, end = notes.times[rows, 0], notes.times[rows, 1]
    pitch, prog = notes.meta[rows, 0].to(torch.int64), notes.meta[rows, 2].to(torch.int64)
    drum, prog = (prog >> 8) & 1, prog & 0xff
    piano = (pitch >= MIN_PITCH) & (pitch <= MAX_PITCH) & (end != start)
    ent_rows, ent_key = [], []
    for name in families:
        f = FAMILIES.index(name)
        if f < 2:
            keep, group = piano, torch.zeros_like(pitch)
        elif name == "flat":
            keep, group = None, drum | drum << 8
        elif name == "midi_class":
            keep, group = None, (prog // 8) * 8 | drum << 8
        else:
            keep, group = None, prog | drum << 8
        key = ((rec * len(FAMILIES) + f) << 9) | group
        ent_rows.append(rows if keep is None else rows[keep])
        ent_key.append(key if keep is None else key[keep])
    # tm._validate: a negative time, a duration <= 0 — among the piano-range notes, and among all
    negative, short = (start < 0) | (end < 0), end <= start
    bad = torch.stack([negative & piano, short & piano, negative, short], 1).to(torch.int64)
    flags = torch.zeros(R, 4, dtype=torch.int64, device=dev).index_add_(0, rec, bad)
    latest = torch.where(torch.isnan(end), torch.zeros_like(end), end).amax() if total else end.new_zeros(())
    return torch.cat(ent_rows), torch.cat(ent_key), flags, latest


def build_problems(ref, est, families=FAMILIES) -> Problems:
    """The lists of `evaluate.py`'s scores for every recording pair (ref recording r against est recording r; `ref`, `est`:
    `mrmt3.notes.DeviceNotes` on one device, the host included).  Per pair:
      - "onoff" and "on": the notes with pitch 21..108 and end != start (`tm.sequence_to_valued_intervals`), pitch table 0,
        the offset criterion on and off;
      - "flat", "midi_class", "full": one problem per (`evaluate.get_granular_program`, is_drum) key present on either side,
        all notes, pitch table 1, offsets off.
    Sorting and counting are torch operations on the tables' device; one tensor comes back: the problem keys, the list
    lengths, the counts that tell where `tm._validate` would raise (`errors`: the same ValueError, per pair), and the
    largest end time (`max_end`)."""
    import torch
    families = tuple(families)
    if not families or any(f not in FAMILIES for f in families):
        raise ValueError("families must be a non-empty subset of %r, got %r" % (FAMILIES, families))
    R = len(ref)
    if len(est) != R:
        raise ValueError("%d reference recordings against %d estimated ones" % (R, len(est)))
    dev = ref.meta.device
    r_rows, r_key, r_flags, r_end = _side(ref, families)
    e_rows, e_key, e_flags, e_end = _side(est, families)
    # the agnostic problems exist for every pair, the group problems where a key is present
    forced = [(r * len(FAMILIES) + FAMILIES.index(f)) << 9 for r in range(R) for f in families if FAMILIES.index(f) < 2]
    # (entries of a problem are in row order: a stable sort by onset leaves onset, then row)
    uniq, ((n_r, r_idx, r_first, (r_low,)), (n_e, e_idx, e_first, (e_low,))) = _lists(
        [(key, rows, torch.sort(notes.times[rows, 0], stable=True).indices, [(rows, "amin", _NO_ROW)])
         for rows, key, notes in ((r_rows, r_key, ref), (e_rows, e_key, est))],
        torch.tensor(forced, dtype=torch.int64, device=dev))
    family_dev = (uniq >> 9) % len(FAMILIES)
    flags = ((family_dev == 0).to(torch.int32) | (torch.where(family_dev < 2, TABLE_MIDI_AS_HZ, TABLE_HZ) << 8)).to(torch.int32)
    uniq_h, n_ref, n_est, first_ref, first_est, bad_ref, bad_est, max_end = _home(
        uniq, n_r, n_e, r_low, e_low, r_flags, e_flags, torch.maximum(r_end, e_end).reshape(1))
    max_end = float(max_end[0])
    family = (uniq_h >> 9) % len(FAMILIES)
    keys = [None if f < 2 else (int(k & 0xff), bool(k >> 8 & 1)) for f, k in zip(family, uniq_h & 0x1ff)]
    piano_only = all(FAMILIES.index(f) < 2 for f in families)
    errors = []
    for r in range(R):
        message = None
        for bad, name in ((bad_ref[r], "reference"), (bad_est[r], "estimated")):
            negative, short = (bad[0], bad[1]) if piano_only else (bad[2], bad[3])
            if message is None and negative:
                message = f"negative {name} interval time"
            if message is None and short:
                message = f"all {name} interval durations must be strictly positive"
        errors.append(None if message is None else ValueError(message))
    return Problems(r_idx, r_first, e_idx, e_first, flags, (uniq_h >> 9) // len(FAMILIES), family, keys,
                    n_ref, n_est, first_ref, first_est, errors, families, max_end)


def assemble_scores(problems: Problems, matched, programs_ref=None, programs_est=None, overlaps=None) -> List[dict]:
    """One dict per recording pair from the matchings' sizes (`matched` [n_prob], host): the keys of
    `evaluate.compute_transcription_metrics` (when "onoff" and "on" were built) and of
    `evaluate.mt3_program_aware_note_scores` at every granularity built, whose "F1 by program" is kept per granularity as
    "F1 by program (<granularity>)" and, for the last of flat / full / midi_class built, as "F1 by program" — what
    `evaluate_main` is left with.  `programs_ref` / `programs_est`: per pair every instrument's (program, is_drum) in order
    (None: the groups in order of first appearance in the table; the same unless an instrument has no notes).
    `overlaps`: {problem: average overlap ratio} for the agnostic problems, or None: the overlap keys are absent."""
    import evaluate
    results = []
    for r, mine in enumerate(problems.by_pair):
        res = {}
        scores = lambda p: tm.scores_from_counts(int(matched[p]), int(problems.n_ref[p]), int(problems.n_est[p]))
        agnostic = {}
        for f in (0, 1):
            if f in mine:
                p = mine[f][0]
                agnostic[f] = scores(p) + (() if overlaps is None else (overlaps[p],))
        if 0 in agnostic and 1 in agnostic:
            p = mine[1][0]
            res.update(evaluate.transcription_metrics_result(int(problems.n_ref[p]), int(problems.n_est[p]), agnostic[0],
                                                             agnostic[1]))
        for name in ("flat", "full", "midi_class"):
            if name not in problems.families:
                continue
            f = FAMILIES.index(name)
            at = {problems.key[p]: p for p in mine.get(f, [])}
            sides = []
            for programs, n, first in ((programs_ref, problems.n_ref, problems.first_ref),
                                       (programs_est, problems.n_est, problems.first_est)):
                if programs is not None and programs[r] is not None:
                    seen = dict.fromkeys((evaluate.get_granular_program(pr, dr, name), bool(dr)) for pr, dr in programs[r])
                    sides.append(list(seen))
                else:
                    sides.append(sorted((k for k, p in at.items() if n[p] > 0), key=lambda k: first[at[k]]))
            groups = []
            for key in evaluate.group_order(sides[0], sides[1]):
                p = at.get(key)
                if p is None:                    # an instrument without notes on either side
                    groups.append((key, (0.0, 0.0, 0.0), 0, 0))
                else:
                    groups.append((key, scores(p), int(problems.n_ref[p]), int(problems.n_est[p])))
            onset = agnostic[1][:3] if 1 in agnostic else (None, None, None)
            got = evaluate.program_aware_result(onset, groups, name)
            if 1 not in agnostic:
                for k in ("Onset precision", "Onset recall", "Onset F1"):
                    del got[k]
            res["F1 by program (%s)" % name] = got["F1 by program"]
            res.update(got)
        results.append(res)
    return results


def upload(tables, device):
    """`DeviceNotes` of a list of tables ((times, meta) pairs, `NoteArrays`, `MidiTable`s), or the argument itself."""
    from mrmt3.notes import DeviceNotes
    return tables if isinstance(tables, DeviceNotes) else DeviceNotes.from_arrays(tables, device)


def frames_for(max_end, fps=FRAMES_PER_SECOND) -> int:
    """The roll length `score_tables` launches with: ceil(max_end * fps) + 1, within the kernel's [1, 2^31 - 64]."""
    import math
    from mrmt3 import lib
    product = float(max_end) * float(fps)
    if not product < lib.FRAMES_MAX:               # (also an infinite end: such notes are skipped, not clipped)
        return lib.FRAMES_MAX
    return max(1, math.ceil(product) + 1)


def add_frame_scores(results, problems: Problems, counts) -> None:
    """The frame keys of every pair's dict from the kernel's (or the host's) `counts` [n_prob, 3]: "Frame precision" /
    "Frame recall" / "Frame F1" from the "on" problem (when built), "Frame F1 (<granularity>)" from the counts summed over
    that granularity's groups (when built).  Assembled where `evaluate.py`'s host path assembles them."""
    import evaluate
    for r, res in enumerate(results):
        if not isinstance(res, dict):
            continue
        on = None
        grouped = {}
        for name in problems.families:
            f = FAMILIES.index(name)
            at = problems.by_pair[r].get(f, [])
            if name == "on":
                on = tuple(int(v) for v in counts[at[0]])
            elif f >= 2:
                grouped[name] = [tuple(int(v) for v in counts[p]) for p in at]
        res.update(evaluate.frame_result(on, grouped))


def add_instrument_scores(results, problems: Problems) -> None:
    """The instrument-detection keys of every pair's dict from the "full" problems' list lengths: no launch."""
    import evaluate
    f = FAMILIES.index("full")
    for r, res in enumerate(results):
        if not isinstance(res, dict):
            continue
        mine = problems.by_pair[r].get(f, [])
        res.update(evaluate.instrument_result([problems.key[p][0] for p in mine if problems.n_ref[p] > 0],
                                              [problems.key[p][0] for p in mine if problems.n_est[p] > 0]))


def _program_key(notes, rows, by):
    import torch
    prog = notes.meta[rows, 2].to(torch.int64)
    return (prog & 0x1ff) if by == "program" else torch.zeros_like(prog)


def pianoroll(notes, fps=FRAMES_PER_SECOND, recording=None, by=None):
    """The piano rolls of a `mrmt3.notes.DeviceNotes`: one bool tensor [frames_r, 128] per recording on the notes' device
    (a list; `recording=r`: that recording's alone), frames_r the largest b of the recording, 0 for a recording
    without notes.  Every note with a pitch in 0..127 is taken.  `by="program"`: per recording a dict
    {(program, is_drum): roll}, every roll of a recording frames_r long.  ONE launch of the frame kernel with the rolls
    written, one problem per roll, unpacked with torch operations; one tensor (the lengths and the keys) comes home."""
    import torch
    from mrmt3 import lib
    if by not in (None, "program"):
        raise ValueError("by must be None or 'program', got %r" % (by,))
    R = len(notes)
    if recording is not None and not 0 <= int(recording) < R:
        raise ValueError("recording %r of %d" % (recording, R))
    dev = notes.meta.device
    rec, rows = notes.entries(recording)
    start, end, pitch = notes.times[rows, 0], notes.times[rows, 1], notes.meta[rows, 0]
    ps, pe = start * fps, end * fps                                   # (one f64 multiplication each, as in the kernel)
    sounds = ~torch.isnan(start) & ~torch.isnan(end) & (pitch >= 0) & (pitch <= 127) & (ps < FRAME_LIMIT) & (pe < FRAME_LIMIT)
    a = torch.floor(ps.clamp(min=0.0))
    b = torch.where(sounds, torch.maximum(a + 1, torch.ceil(pe.clamp(min=0.0))), torch.zeros_like(a)).to(torch.int64)
    key = (rec << 9) | _program_key(notes, rows, by)
    wanted = range(R) if recording is None else [int(recording)]
    forced = torch.tensor([r << 9 for r in wanted] if by is None else [], dtype=torch.int64, device=dev)
    uniq, ((_, idx, first, (last,)),) = _lists([(key, rows, None, [(b, "amax", 0)])], forced)
    P = int(uniq.numel())
    if P == 0:                                       # by="program" without a single note
        return [dict() for _ in wanted] if recording is None else dict()
    uniq_h, last_h = _home(uniq, last)
    frames = {int(r): 0 for r in wanted}
    for k, v in zip(uniq_h >> 9, last_h):
        frames[int(k)] = max(frames[int(k)], int(v))
    n_frames = max(1, max(frames.values()))
    if n_frames > lib.FRAMES_MAX:
        raise ValueError("a piano roll of %d frames is beyond the kernel's 2^31 - 64" % n_frames)
    none = torch.zeros(P + 1, dtype=torch.int32, device=dev)
    _, _, clipped, roll = lib.note_frames(notes.times, notes.meta, notes.times, notes.meta, idx, first,
                                          none[:0], none, fps, n_frames, with_roll=True)
    bits = (roll[:, 0].unsqueeze(-1) >> torch.arange(32, device=dev, dtype=torch.int32)) & 1      # [P, 128, W, 32]
    dense = bits.reshape(P, 128, -1).transpose(1, 2).to(torch.bool)                                # [P, W * 32, 128]
    out = {int(r): ({} if by else None) for r in wanted}
    for p, k in enumerate(uniq_h.tolist()):
        r = k >> 9
        piece = dense[p, :frames[r]]
        if by is None:
            out[r] = piece
        else:
            out[r][(k & 0xff, bool(k >> 8 & 1))] = piece
    got = [out[int(r)] for r in wanted]
    return got if recording is None else got[0]


def score_tables(ref, est, with_overlap=False, families=FAMILIES, errors="raise", device=None, return_matching=False,
                 frames=False, instruments=False, fps=FRAMES_PER_SECOND):
    """ref, est: `mrmt3.notes.DeviceNotes` (or lists of tables, uploaded to `device`) -> one dict per recording pair with the
    keys of `compute_transcription_metrics` and of `mt3_program_aware_note_scores` at the three granularities (see
    `assemble_scores`), from ONE launch of the device matcher for all pairs and all problems.  Only `matched`, the list
    lengths and `status` come back; with `with_overlap` also `match` and what `tm.average_overlap_ratio` of the kernel's
    matching needs, and the overlap keys are present.  `families`: the scores to build (a subset of FAMILIES).
    A pair the host scorer would refuse raises its ValueError (`errors="return"`: the pair's entry is the exception).
    `return_matching` (with `with_overlap`): also returns, per pair, {"onoff": pairs, "on": pairs}, the kernel's matchings
    as sorted (reference note, estimated note) numbers within the recording.
    `frames`: ONE launch more, of the frame kernel over the same problems at `fps`; its counts come home in the
    tensor `matched` comes home in, and every pair's dict gains "Frame precision" / "Frame recall" / "Frame F1" (the lists
    of the "on" problem) and "Frame F1 (<granularity>)" for the granularities built.  `instruments`: the instrument-detection
    keys of `evaluate.instrument_result` from the "full" problems' list lengths, no launch.  Both off: what it always did."""
    import torch
    from mrmt3 import lib
    families = tuple(families)
    if instruments and "full" not in families:
        raise ValueError("instruments=True counts the program sets of the 'full' problems: families %r lack them" % (families,))
    if device is None:
        device = ref.meta.device if hasattr(ref, "first") else est.meta.device if hasattr(est, "first") else "cuda"
    programs = [[getattr(t, "programs", None) for t in side] if isinstance(side, (list, tuple)) else None for side in (ref, est)]
    ref, est = upload(ref, device), upload(est, device)
    problems = build_problems(ref, est, families)
    if errors == "raise":
        for e in problems.errors:
            if e is not None:
                raise e
    key = str(ref.meta.device)
    if key not in _PITCH_TABLES:
        _PITCH_TABLES[key] = tuple(torch.from_numpy(t).to(ref.meta.device) for t in pitch_tables())
    lo, hi = _PITCH_TABLES[key]
    matched, match, status = lib.note_match(ref.times, ref.meta, est.times, est.meta, problems.ref_idx, problems.ref_first,
                                            problems.est_idx, problems.est_first, problems.prob_flags, lo, hi, ONSET_TOLERANCE,
                                            OFFSET_RATIO, OFFSET_MIN_TOLERANCE)
    if frames:
        counts, _, clipped = lib.note_frames(ref.times, ref.meta, est.times, est.meta, problems.ref_idx, problems.ref_first,
                                             problems.est_idx, problems.est_first, fps, frames_for(problems.max_end, fps))
        matched, status, frame_counts, clipped = _home(matched, status, counts, clipped)
        # (a pair the host scorer refuses may hold a note that starts after the last end: its problems are not scored)
        scored = np.asarray([problems.errors[int(r)] is None for r in problems.pair], bool)
        if clipped[scored].any():
            raise RuntimeError("note_frames: clipped %r although n_frames came from the same tables" % clipped.tolist())
    else:
        matched, status = _home(matched, status)
    if status.any():
        raise RuntimeError("note_match: status %r (the lists of build_problems are in order: a NaN onset?)" % status.tolist())
    overlaps = matchings = None
    if with_overlap:
        overlaps, matchings = _overlaps(problems, ref, est, match)
    out = assemble_scores(problems, matched, programs[0], programs[1], overlaps)
    if frames:
        add_frame_scores(out, problems, frame_counts)
    if instruments:
        add_instrument_scores(out, problems)
    out = [problems.errors[r] if problems.errors[r] is not None else out[r] for r in range(len(out))]
    return (out, matchings) if return_matching else out


_PITCH_TABLES = {}


def _overlaps(problems, ref, est, match):
    """({agnostic problem: `tm.average_overlap_ratio` of the kernel's matching}, per pair {"onoff" / "on": the matching}),
    pairs in (reference row, estimated row) order as `tm.match_notes` returns them."""
    match = match.cpu().numpy()
    ref_idx, est_idx = problems.ref_idx.cpu().numpy(), problems.est_idx.cpu().numpy()
    est_first = problems.est_first.cpu().numpy()
    ref_times, est_times = ref.times.cpu().numpy(), est.times.cpu().numpy()
    ref_at, est_at = ref.first.cpu().numpy(), est.first.cpu().numpy()
    out, matchings = {}, [dict() for _ in problems.errors]
    for p in np.flatnonzero(problems.family < 2):
        pairs = matching_of(p, match, ref_idx, est_idx, est_first)
        r = int(problems.pair[p])
        matchings[r][FAMILIES[problems.family[p]]] = [(a - int(ref_at[r]), b - int(est_at[r])) for a, b in pairs]
        if problems.n_ref[p] == 0 or problems.n_est[p] == 0:
            out[p] = 0.0
        else:
            out[p] = tm.average_overlap_ratio(ref_times, est_times, pairs)
    return out, matchings


def matching_of(p, match, ref_idx, est_idx, est_first):
    """Sorted (reference row, estimated row) pairs of problem p from the kernel's `match`."""
    k = np.arange(int(est_first[p]), int(est_first[p + 1]))
    k = k[match[k] >= 0]
    return sorted(zip(ref_idx[match[k]].tolist(), est_idx[k].tolist()))
