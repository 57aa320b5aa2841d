"""Shared material of the frame-score tests: the seeded corpus, the hand-written boundary and union cases, and
the grid times at which the f64 product and the exact quotient disagree.  A case is (ref, est): each side a list of
(start, end, pitch); `pack` lays cases end to end as one launch, one problem per case."""
import dataclasses
from fractions import Fraction

import numpy as np

N_CASES = 320


@dataclasses.dataclass
class Packed:
    ref_times: np.ndarray
    ref_meta: np.ndarray
    est_times: np.ndarray
    est_meta: np.ndarray
    ref_idx: np.ndarray
    ref_first: np.ndarray
    est_idx: np.ndarray
    est_first: np.ndarray

    def arrays(self):
        return (self.ref_times, self.ref_meta, self.est_times, self.est_meta, self.ref_idx, self.ref_first, self.est_idx,
                self.est_first)


def _table(notes):
    times = np.asarray([(s, e) for s, e, _ in notes], np.float64).reshape(-1, 2)
    meta = np.zeros((len(notes), 4), np.int32)
    meta[:, 0] = [p for _, _, p in notes]
    meta[:, 1] = 90
    return times, meta


def pack(cases, seed=5) -> Packed:
    """The cases' notes as two tables and the problems' lists, each list in a seeded random order (no order is promised)."""
    rng = np.random.default_rng(seed)
    tables, idx, first = [[], []], [[], []], [[0], [0]]
    at = [0, 0]
    for case in cases:
        for s in (0, 1):
            notes = case[s]
            tables[s].extend(notes)
            idx[s].extend((at[s] + rng.permutation(len(notes))).tolist())
            at[s] += len(notes)
            first[s].append(at[s])
    (rt, rm), (et, em) = _table(tables[0]), _table(tables[1])
    return Packed(rt, rm, et, em, np.asarray(idx[0], np.int32), np.asarray(first[0], np.int32), np.asarray(idx[1], np.int32),
                  np.asarray(first[1], np.int32))


def _side(rng, n, base, n_pitch, span):
    start = rng.integers(0, span, n) * 0.01 + rng.uniform(-0.004, 0.004, n)
    start = np.maximum(start, 0.0)
    dur = rng.integers(0, 61, n) * 0.01
    return [(float(s), float(s + d), int(base + q)) for s, d, q in zip(start, dur, rng.integers(0, n_pitch, n))]


def corpus():
    """N_CASES problems: 0..40 notes a side on the 10 ms grid with +-4 ms jitter, 3..6 pitches, durations of 0..0.6 s: notes
    of one pitch overlap and zero lengths occur."""
    rng = np.random.default_rng(20250314)
    cases = []
    for _ in range(N_CASES):
        n_ref, n_est = (int(v) for v in rng.integers(0, 41, 2))
        n_pitch, base, span = int(rng.integers(3, 7)), int(rng.integers(0, 122)), int(rng.integers(6, 400))
        cases.append((_side(rng, n_ref, base, n_pitch, span), _side(rng, n_est, base, n_pitch, span)))
    return cases


def start_at(f, fps):
    """A start time whose frame a is f whatever the last bit of the product: a quarter of a frame inside it."""
    t = (f + 0.25) / fps
    assert np.floor(np.float64(t) * np.float64(fps)) == f
    return t


def end_at(f, fps):
    """An end time whose frame b is f: a quarter of a frame before the frame border."""
    t = (f - 0.25) / fps
    assert np.ceil(np.float64(t) * np.float64(fps)) == f
    return t


def boundary_cases(tile, fps):
    """One-note and two-note problems against the kernel's constants -> (cases, expected): expected[i] is (tp, n_ref, n_est).
    Times are built from frame numbers, so the same cases exist at every fps."""
    s, e = (lambda f: start_at(f, fps)), (lambda f: end_at(f, fps))
    cases, want = [], []

    def add(ref, est, expect=None):
        cases.append((ref, est))
        want.append(expect)

    for edge in (32, tile):                      # a and b at the word edges and at the tile edges
        for a in (edge - 1, edge, edge + 1):
            add([(s(a), e(a + 5), 60)], [(s(a), e(a + 5), 60)], (5, 5, 5))
        for b in (edge - 1, edge, edge + 1):
            add([(s(3), e(b), 60)], [(s(2), e(b), 60)], (b - 3, b - 3, b - 2))
    add([(s(tile - 7), e(4 * tile + 9), 64)], [(s(tile), e(4 * tile), 64)], (3 * tile, 3 * tile + 16, 3 * tile))
    add([(s(tile), e(4 * tile), 0)], [(s(tile), e(4 * tile), 127)], (0, 3 * tile, 3 * tile))    # three whole tiles
    add([(s(35), e(39), 60)], [(s(36), e(38), 60)], (2, 4, 2))              # wholly inside one word
    add([(s(10), s(10), 60)], [(s(10), e(11), 60)], (1, 1, 1))              # end == start: one frame
    add([(s(50), e(20), 60)], [(s(50), e(51), 60)], (1, 1, 1))              # end < start: one frame at a
    add([(-1.0, e(4), 60)], [(0.0, e(4), 60)], (4, 4, 4))                   # start < 0
    add([(-2.0, -1.0, 60)], [], (0, 1, 0))                                  # all of it before 0: frame 0
    for pitch in (-1, 0, 127, 128):
        ok = int(0 <= pitch <= 127)
        add([(s(1), e(3), pitch)], [(s(1), e(3), pitch)], (2 * ok, 2 * ok, 2 * ok))
    add([(float("nan"), 1.0, 60), (s(0), e(2), 60)], [(1.0, float("nan"), 60)], (0, 2, 0))
    add([(0.0, 1e300, 60)], [(1e300, 1e300, 60), (s(0), e(1), 60)], (0, 0, 1))
    add([(0.0, float("inf"), 60)], [(-float("inf"), e(2), 60)], (0, 0, 2))
    return cases, want


def disagreeing_grid_times(fps=62.5, limit=100000, count=20):
    """The first `count` k for which floor((k * 0.01) * fps) in f64 differs from the floor of the exact k * fps / 100."""
    found = []
    for k in range(limit):
        exact = (Fraction(k) * Fraction(fps) / 100).__floor__()
        if int(np.floor(np.float64(k * 0.01) * np.float64(fps))) != exact:
            found.append((k, exact))
            if len(found) == count:
                break
    return found


def union_cases():
    """(cases, expected counts) with closed forms, at 62.5 fps."""
    s, e = (lambda f: start_at(f, 62.5)), (lambda f: end_at(f, 62.5))
    one = [(s(100), e(140), 60), (s(120), e(160), 60)]           # two references of one pitch, overlapping by half
    cases = [(one, [(s(90), e(170), 60)]),
             (one + [(s(5), e(9), 72)], list(one) + [(s(5), e(9), 72)]),
             ([(s(0), e(40), 60)], [(s(0), e(40), 61)]),
             ([], [(s(0), e(40), 61)]),
             ([(s(0), e(40), 61)], []),
             ([], [])]
    want = [(60, 60, 80), (64, 64, 64), (0, 40, 40), (0, 0, 40), (0, 40, 0), (0, 0, 0)]
    return cases, want


def dense_roll(notes, fps, n_frames):
    """bool [n_frames, 128] of a list of (start, end, pitch): the definition, note by note, in Python floats."""
    import math
    roll = np.zeros((n_frames, 128), bool)
    for start, end, pitch in notes:
        if start != start or end != end or not 0 <= pitch <= 127 or not start * fps < 2.0 ** 31 or not end * fps < 2.0 ** 31:
            continue
        a = max(0, math.floor(start * fps)) if start * fps > -1e18 else 0
        b = max(a + 1, math.ceil(end * fps) if end * fps > -1e18 else 0)
        roll[min(a, n_frames):min(b, n_frames), pitch] = True
    return roll


def _union(intervals):
    """Disjoint sorted [a, b) intervals with the same union."""
    out = []
    for a, b in sorted(intervals):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def frame_counts_intervals(ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first,
                           fps=62.5, n_frames=1):
    """`scoring.frame_counts_host` without a roll, a second, independent form: per pitch the length of the union of each
    side's [a, b) intervals and of the intersection of the two unions, in Python floats and ints -> (counts, skipped,
    clipped).  Only the range clamp is the product's."""
    import math
    from mrmt3.scoring import FRAME_LIMIT, _clamped
    n_prob, n_frames, fps = len(ref_first) - 1, int(n_frames), float(fps)
    counts = np.zeros((n_prob, 3), np.int64)
    skipped, clipped = np.zeros((n_prob, 2), np.int32), np.zeros((n_prob, 2), np.int32)
    sides = ((np.asarray(ref_times, np.float64).reshape(-1, 2).tolist(), np.asarray(ref_meta).reshape(-1, 4)[:, 0].tolist(),
              ref_idx, ref_first),
             (np.asarray(est_times, np.float64).reshape(-1, 2).tolist(), np.asarray(est_meta).reshape(-1, 4)[:, 0].tolist(),
              est_idx, est_first))
    for p in range(n_prob):
        rows = [dict(), dict()]                      # per side: pitch -> intervals
        for s, (times, pitches, idx, first) in enumerate(sides):
            lo, hi = _clamped(first, p, max(int(first[n_prob]), 0))
            for note in (int(i) for i in idx[lo:hi]):
                if note < 0 or note >= len(times):
                    skipped[p, s] += 1
                    continue
                (start, end), pitch = times[note], pitches[note]
                ps, pe = start * fps, end * fps
                if start != start or end != end or pitch < 0 or pitch > 127 or not ps < FRAME_LIMIT or not pe < FRAME_LIMIT:
                    skipped[p, s] += 1
                    continue
                a = 0 if ps < 0 else math.floor(ps)
                b = max(a + 1, 0 if pe < 0 else math.ceil(pe))
                if b > n_frames:
                    clipped[p, s] += 1
                    b = n_frames
                if a < b:
                    rows[s].setdefault(pitch, []).append((a, b))
        for s in (0, 1):
            rows[s] = {q: _union(iv) for q, iv in rows[s].items()}
            counts[p, 1 + s] = sum(b - a for iv in rows[s].values() for a, b in iv)
        for q in set(rows[0]) & set(rows[1]):
            x, y, i, j = rows[0][q], rows[1][q], 0, 0
            while i < len(x) and j < len(y):
                counts[p, 0] += max(0, min(x[i][1], y[j][1]) - max(x[i][0], y[j][0]))
                if x[i][1] <= y[j][1]:
                    i += 1
                else:
                    j += 1
    return counts, skipped, clipped
