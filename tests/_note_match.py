"""Shared material of the note-matching tests: the seeded corpus, the dense graph of
`contrib.transcription_metrics.match_notes`, first-fit matchings, chains, and synthetic MIDI data."""
import dataclasses

import numpy as np

from contrib import midi_io
from contrib import transcription_metrics as tm

N_CASES = 360


@dataclasses.dataclass
class Case:
    ref_times: np.ndarray
    ref_meta: np.ndarray
    est_times: np.ndarray
    est_meta: np.ndarray
    offsets: bool
    table: int
    onset_tol: float = 0.05

    @property
    def flags(self):
        return int(self.offsets) | self.table << 8


def _notes(rng, n, base, n_pitch, span):
    onset = rng.integers(0, span, n) * 0.01
    jitter = rng.random(n) < 0.3
    onset = np.abs(onset + jitter * rng.normal(0.0, 2e-3, n))
    times = np.stack([onset, onset + rng.integers(1, 20, n) * 0.01], 1).reshape(-1, 2)
    meta = np.zeros((n, 4), np.int32)
    meta[:, 0] = base + rng.integers(0, n_pitch, n)
    meta[:, 1] = rng.integers(1, 128, n)
    return times, meta


def corpus():
    """N_CASES cases: 0..40 notes per side, onsets on the 10 ms grid (three in ten jittered by about 2 ms), 3 to 6 pitches,
    the offset criterion on and off, both pitch tables."""
    rng = np.random.default_rng(20240611)
    cases = []
    for c in range(N_CASES):
        n_ref, n_est = (int(v) for v in rng.integers(0, 41, 2))
        n_pitch, base, span = int(rng.integers(3, 7)), int(rng.integers(36, 100)), int(rng.integers(6, 40))
        cases.append(Case(*_notes(rng, n_ref, base, n_pitch, span), *_notes(rng, n_est, base, n_pitch, span),
                          offsets=bool(c // 2 % 2), table=c % 2))
    return cases


def matcher_pitches(case):
    """The pitch arrays `evaluate.py` hands to the matcher for the case's table."""
    ref, est = case.ref_meta[:, 0].astype(np.float64), case.est_meta[:, 0].astype(np.float64)
    return (tm.midi_to_hz(ref), tm.midi_to_hz(est)) if case.table else (ref, est)


def dense_hit(case):
    """bool [n_ref, n_est]: the adjacency of `tm.match_notes`, by its own dense expressions."""
    ref, est = case.ref_times, case.est_times
    ref_p, est_p = matcher_pitches(case)
    hit = np.around(np.abs(np.subtract.outer(ref[:, 0], est[:, 0])), decimals=6) <= case.onset_tol
    with np.errstate(divide="ignore", invalid="ignore"):
        hit &= np.abs(1200.0 * np.subtract.outer(np.log2(ref_p), np.log2(est_p))) <= 50.0
    if case.offsets:
        off = np.around(np.abs(np.subtract.outer(ref[:, 1], est[:, 1])), decimals=6)
        hit &= off <= np.maximum(0.2 * (ref[:, 1] - ref[:, 0]), 0.05).reshape(-1, 1)
    return hit


def host_size(case):
    """The size of `tm.match_notes`' matching (0 for an empty side, where the host scorer does not call it)."""
    if not len(case.ref_meta) or not len(case.est_meta):
        return 0
    ref_p, est_p = matcher_pitches(case)
    return len(tm.match_notes(case.ref_times, ref_p, case.est_times, est_p, onset_tolerance=case.onset_tol,
                              offset_ratio=0.2 if case.offsets else None))


def lists(case):
    """(ref_idx, est_idx): each side in onset order, equal onsets by index."""
    return (np.argsort(case.ref_times[:, 0], kind="stable").astype(np.int32),
            np.argsort(case.est_times[:, 0], kind="stable").astype(np.int32))


def first_fit(hit, est_order, highest):
    """The size of the matching without augmentation: every estimated note, in `est_order`, takes its lowest (highest) free
    reference in list order.  `hit` is [ref position, est position] over the sorted lists."""
    taken, size = np.zeros(hit.shape[0], bool), 0
    for e in est_order:
        free = np.flatnonzero(hit[:, e] & ~taken)
        if len(free):
            taken[free[-1 if highest else 0]] = True
            size += 1
    return size


@dataclasses.dataclass
class Packed:
    """Several cases as one launch: the tables end to end, one problem per case."""
    ref_times: np.ndarray
    ref_meta: np.ndarray
    est_times: np.ndarray
    est_meta: np.ndarray
    ref_idx: np.ndarray
    ref_first: np.ndarray
    est_idx: np.ndarray
    est_first: np.ndarray
    flags: np.ndarray
    ref_at: np.ndarray                           # every case's first row in the tables
    est_at: np.ndarray

    def arrays(self):
        return (self.ref_times, self.ref_meta, self.est_times, self.est_meta, self.ref_idx, self.ref_first, self.est_idx,
                self.est_first, self.flags)


def pack(cases) -> Packed:
    ref_idx, est_idx, ref_first, est_first, r_at, e_at, ref_at, est_at = [], [], [0], [0], 0, 0, [], []
    for c in cases:
        r, e = lists(c)
        ref_idx.append(r + r_at)
        est_idx.append(e + e_at)
        ref_at.append(r_at)
        est_at.append(e_at)
        r_at += len(r)
        e_at += len(e)
        ref_first.append(r_at)
        est_first.append(e_at)
    cat = lambda parts, shape, dtype: np.concatenate([np.zeros(0, dtype).reshape(shape)]
                                                     + [np.asarray(p, dtype).reshape(shape) for p in parts])
    return Packed(cat([c.ref_times for c in cases], (-1, 2), np.float64), cat([c.ref_meta for c in cases], (-1, 4), np.int32),
                  cat([c.est_times for c in cases], (-1, 2), np.float64), cat([c.est_meta for c in cases], (-1, 4), np.int32),
                  cat(ref_idx, (-1,), np.int32), np.asarray(ref_first, np.int32), cat(est_idx, (-1,), np.int32),
                  np.asarray(est_first, np.int32), np.asarray([c.flags for c in cases], np.int32), np.asarray(ref_at),
                  np.asarray(est_at))


def check_matching(packed, cases, matched, match):
    """`match` holds, for every problem, a valid matching of `matched[p]` pairs: each pair an edge of the dense graph, no
    reference used twice, partners inside the problem's own list."""
    for p, c in enumerate(cases):
        hit = dense_hit(c)
        r0, r1, e0, e1 = packed.ref_first[p], packed.ref_first[p + 1], packed.est_first[p], packed.est_first[p + 1]
        got = match[e0:e1]
        used = got[got >= 0]
        assert len(used) == matched[p], (p, len(used), matched[p])
        assert ((used >= r0) & (used < r1)).all(), p
        assert len(set(used.tolist())) == len(used), p
        for k in np.flatnonzero(got >= 0):
            assert hit[packed.ref_idx[got[k]] - packed.ref_at[p], packed.est_idx[e0 + k] - packed.est_at[p]], (p, k)


BOUNDARY = [0.05, 0.0500004, 0.0500006, 0.049999, 0.06]


def boundary_cases():
    """1 x 1 problems at every boundary value: the 500 grid differences |(a + 0.05) - a|, a = k * 0.01, and onset and offset
    differences just inside and just outside the tolerance."""
    meta = np.asarray([[60, 100, 0, 0]], np.int32)
    cases = []
    for k in range(500):
        a = k * 0.01
        cases.append(Case(np.asarray([[a + 0.05, a + 1.0]]), meta, np.asarray([[a, a + 1.0]]), meta, False, 1))
    for d in BOUNDARY:
        for sign in (1.0, -1.0):
            cases.append(Case(np.asarray([[1.0 + sign * d, 3.0]]), meta, np.asarray([[1.0, 3.0]]), meta, False, 1))
            # a 0.1 s reference: the offset tolerance is max(0.2 * 0.1, 0.05) = 0.05
            cases.append(Case(np.asarray([[1.0, 1.1]]), meta, np.asarray([[1.0, 1.1 + sign * d]]), meta, True, 1))
    return cases


# The chains run at an onset tolerance of 0.04: with e_i at 0.04 i and r_j at 0.04 j + 0.03 the distances to r_{i-1} and
# r_i are 0.01 and 0.03, and the next one, to r_{i-2}, is 0.05 exactly after the rounding — at the default tolerance it
# would be a third neighbour and the closed forms below would not hold.
CHAIN_TOL = 0.04


def chain(n, keep_first, keep_last, mirror):
    """e_i at 0.04 i (i < n) and r_j at 0.04 j + 0.03 for j in -1 .. n - 1, so e_i is adjacent to r_{i-1} and r_i; the
    spare references r_{-1} / r_{n-1} kept or removed; `mirror`: time runs backwards.  Returns (case, size, unique), `unique`
    the only maximum matching as {est index: ref index} or None."""
    js = np.arange(-1 if keep_first else 0, n if keep_last else n - 1)
    est_on, ref_on = 0.04 * np.arange(n), 0.04 * js + 0.03
    if mirror:
        est_on, ref_on = 0.04 * n - est_on, 0.04 * n - ref_on
    meta = lambda m: np.tile(np.asarray([[60, 100, 0, 0]], np.int32), (m, 1))
    case = Case(np.stack([ref_on, ref_on + 0.5], 1), meta(len(js)), np.stack([est_on, est_on + 0.5], 1), meta(n), False, 1,
                onset_tol=CHAIN_TOL)
    size = n if (keep_first or keep_last) else n - 1
    unique = None
    if keep_first != keep_last:                  # e_0 forced onto r_0, or e_{n-1} onto r_{n-2}: the rest follows
        unique = {i: i for i in range(n)}        # (r_{i-1} or r_i: row i of the reference table either way)
    return case, size, unique


def midi(groups):
    """MidiData from [(program, is_drum, [(start, end, pitch), ...]), ...]."""
    insts = [midi_io.MidiInstrument(program, drum, [midi_io.MidiNote(s, e, p, 90) for s, e, p in notes])
             for program, drum, notes in groups]
    end = max([n.end for i in insts for n in i.notes] or [0.0])
    return midi_io.MidiData(insts, 220, end)


def synthetic_midi(seed, n=60, zero_length=False, drop=0.2, extra=0.2):
    """A reference and an estimate of it: drums, three programs in two General-MIDI families (0, 1 and 40), notes outside
    21..108, optionally a zero-length note; the estimate loses and gains notes and its times move by up to 60 ms."""
    rng = np.random.default_rng(seed)
    programs = [(0, False), (1, False), (40, False), (0, True)]
    ref = [[] for _ in programs]
    for _ in range(n):
        g = int(rng.integers(0, len(programs)))
        start = float(rng.integers(0, 400)) * 0.01
        pitch = int(rng.choice([12, 20, 21, 60, 61, 62, 84, 108, 109, 120]))
        ref[g].append((start, start + float(rng.integers(1, 40)) * 0.01, pitch))
    est = [[] for _ in programs]
    for g, notes in enumerate(ref):
        for s, e, p in notes:
            if rng.random() < drop:
                continue
            move = float(rng.integers(-6, 7)) * 0.01
            s2 = max(0.0, s + move)
            est[g if rng.random() < 0.9 else (g + 1) % 3].append((s2, max(s2 + 0.01, e + float(rng.integers(-6, 7)) * 0.01), p))
        for _ in range(int(extra * len(notes))):
            s = float(rng.integers(0, 400)) * 0.01
            est[g].append((s, s + 0.1, int(rng.choice([60, 61, 84]))))
    if zero_length:
        ref[1].append((1.0, 1.0, 60))
    order = [2, 0, 3, 1]                         # the estimate lists its instruments in another order
    return (midi([(programs[g][0], programs[g][1], ref[g]) for g in range(len(programs))]),
            midi([(programs[g][0], programs[g][1], est[g]) for g in order]))
