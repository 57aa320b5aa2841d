"""Note matching without a GPU: the host restatement of `mrmt3_note_match_fwd` against
`contrib.transcription_metrics.match_notes` and scipy's maximum bipartite matching over the seeded corpus of
tests/_note_match.py, the rounding of the distances, the pitch tables, `build_problems` + `assemble_scores` against
`evaluate.py`, and the C ABI's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _note_match as M  # noqa: E402

import evaluate  # noqa: E402
from contrib import transcription_metrics as tm  # noqa: E402
from mrmt3 import lib, scoring  # noqa: E402
from mrmt3.notes import DeviceNotes  # noqa: E402


@pytest.fixture(scope="module")
def corpus():
    return M.corpus()


@pytest.fixture(scope="module")
def tables():
    return scoring.pitch_tables()


def _host(cases, tables, **tol):
    packed = M.pack(cases)
    return packed, scoring.match_notes_host(*packed.arrays(), *tables, **tol)


def test_host_matcher_equals_the_dense_matcher_and_scipy(corpus, tables):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    assert len(corpus) >= 300
    packed, (matched, match, status) = _host(corpus, tables)
    assert not status.any()
    M.check_matching(packed, corpus, matched, match)
    for p, case in enumerate(corpus):
        assert matched[p] == M.host_size(case), p
        hit = M.dense_hit(case)
        best = maximum_bipartite_matching(csr_matrix(hit), perm_type="column") if hit.size else np.zeros(0)
        assert matched[p] == int((best >= 0).sum()), p
    assert {(c.offsets, c.table) for c in corpus} == {(a, b) for a in (False, True) for b in (0, 1)}
    assert any(len(c.ref_meta) == 0 for c in corpus) and any(len(c.est_meta) == 0 for c in corpus)


def test_corpus_defeats_every_first_fit(corpus, tables):
    """Matching without augmentation, in each of its four orders, falls short of the maximum in at least 20 cases: a
    kernel that only takes free references cannot pass the corpus."""
    _, (matched, _, _) = _host(corpus, tables)
    short = {(rev, high): 0 for rev in (False, True) for high in (False, True)}
    for p, case in enumerate(corpus):
        r, e = M.lists(case)
        hit = M.dense_hit(case)[np.ix_(r, e)]
        for rev, high in short:
            order = range(len(e) - 1, -1, -1) if rev else range(len(e))
            size = M.first_fit(hit, order, high)
            assert size <= matched[p]
            short[rev, high] += size < matched[p]
    assert min(short.values()) >= 20, short


def test_distances_are_rounded_as_numpy_rounds_them(tables):
    cases = M.boundary_cases()
    grid, rest = cases[:500], cases[500:]
    raw = sum(abs(c.ref_times[0, 0] - c.est_times[0, 0]) <= 0.05 for c in grid)
    assert raw == 341                            # the unrounded comparison loses a third of the exact 50 ms differences
    _, (matched, _, status) = _host(cases, tables)
    assert not status.any() and (matched[:500] == 1).all()
    want = []
    for d in M.BOUNDARY:
        want += [int(round(d, 6) <= 0.05)] * 4   # onset and offset, either side
    assert want == [1] * 8 + [0] * 4 + [1] * 4 + [0] * 4
    assert matched[500:].tolist() == want
    assert matched[500:].tolist() == [int(M.dense_hit(c)[0, 0]) for c in rest]


def test_pitch_tables_are_the_dense_cents_matrix(tables):
    lo, hi = tables
    assert lo.shape == hi.shape == (2, 128) and lo.dtype == hi.dtype == np.int32
    midi = np.arange(128, dtype=np.float64)
    for t, values in ((0, midi), (1, tm.midi_to_hz(midi))):
        with np.errstate(divide="ignore", invalid="ignore"):
            hit = np.abs(1200.0 * np.subtract.outer(np.log2(values), np.log2(values))) <= 50.0
        if t == 0:
            hit[0, :] = hit[:, 0] = False
        e = np.arange(128)
        assert ((lo[t][:, None] <= e[None, :]) & (e[None, :] <= hi[t][:, None]) == hit).all()
    assert (lo[1] == np.arange(128)).all() and (hi[1] == np.arange(128)).all()
    assert (lo[0, 60], hi[0, 60], lo[0, 84], hi[0, 84], lo[0, 108], hi[0, 108]) == (59, 61, 82, 86, 105, 111)
    assert all(lo[0, p] == hi[0, p] == p for p in range(1, 35)) and lo[0, 0] > hi[0, 0]


def test_unordered_lists_and_edge_less_entries(tables):
    case = M.corpus()[5]
    packed = M.pack([case, case, case])
    n = len(case.est_meta)
    assert n >= 2 and len(case.ref_meta) >= 2
    want = scoring.match_notes_host(*M.pack([case]).arrays(), *tables)[0][0]
    # problem 1 with its first and last estimated entries swapped
    e0 = packed.est_first[1]
    packed.est_idx[[e0, e0 + n - 1]] = packed.est_idx[[e0 + n - 1, e0]]
    matched, match, status = scoring.match_notes_host(*packed.arrays(), *tables)
    assert status.tolist() == [0, 2, 0] and matched.tolist() == [want, 0, want]
    assert (match[e0:e0 + n] == -1).all()
    # indices outside the table and NaN onsets have no edges and do not disturb the order
    packed = M.pack([case])
    packed.est_idx[1] = len(case.est_meta) + 7
    packed.ref_idx[0] = -3
    packed.ref_times[packed.ref_idx[1], 0] = np.nan
    matched, match, status = scoring.match_notes_host(*packed.arrays(), *tables)
    assert status.tolist() == [0] and match[1] == -1 and not np.isin(match, [0, 1]).any()
    keep_r, keep_e = np.ones(len(case.ref_meta), bool), np.ones(n, bool)
    keep_r[M.lists(case)[0][:2]] = False
    keep_e[M.lists(case)[1][1]] = False
    rest = M.Case(case.ref_times[keep_r], case.ref_meta[keep_r], case.est_times[keep_e], case.est_meta[keep_e], case.offsets,
                  case.table)
    assert matched[0] == M.host_size(rest)


def _notes_of(mids, dev="cpu"):
    return DeviceNotes.from_arrays([scoring.table_from_midi(m) for m in mids], dev)


def _host_scores(pairs, families=scoring.FAMILIES):
    """build_problems on host tensors + the host matcher + assemble_scores."""
    tabs = [[scoring.table_from_midi(m) for m in side] for side in zip(*pairs)]
    ref, est = _notes_of([r for r, _ in pairs]), _notes_of([e for _, e in pairs])
    problems = scoring.build_problems(ref, est, families)
    for e in problems.errors:
        if e is not None:
            raise e
    matched, _, status = scoring.match_notes_host(
        ref.times.numpy(), ref.meta.numpy(), est.times.numpy(), est.meta.numpy(), problems.ref_idx.numpy(),
        problems.ref_first.numpy(), problems.est_idx.numpy(), problems.est_first.numpy(), problems.prob_flags.numpy(),
        *scoring.pitch_tables())
    assert not status.any()
    return scoring.assemble_scores(problems, matched, [t.programs for t in tabs[0]], [t.programs for t in tabs[1]])


def expected_scores(ref, est):
    """What `evaluate.py` gives for one pair, in the key layout of `assemble_scores` (overlap keys left out)."""
    want = {k: v for k, v in evaluate.compute_transcription_metrics(ref, est).items() if "overlap" not in k}
    for g in ("flat", "full", "midi_class"):
        got = evaluate.mt3_program_aware_note_scores(ref, est, g)
        want["F1 by program (%s)" % g] = got["F1 by program"]
        want.update(got)
    return want


def test_build_problems_reproduces_evaluate():
    pairs = [M.synthetic_midi(s) for s in (1, 2, 3)]
    pairs.append((pairs[0][0], M.midi([])))                                       # nothing transcribed
    pairs.append((M.midi([(5, False, []), (0, True, [(0.5, 0.6, 38)])]), pairs[1][1]))  # an instrument without notes
    got = _host_scores(pairs)
    for (ref, est), mine in zip(pairs, got):
        want = expected_scores(ref, est)
        assert set(mine) == set(want)
        for k in want:
            assert mine[k] == want[k], (k, mine[k], want[k])
    assert 0 < got[0]["Onset + program F1 (full)"] < got[0]["Onset + program F1 (flat)"] < 1 and 0 < got[0]["Onset F1"] < 1
    assert got[0]["len_ref_intervals"] < sum(len(i.notes) for i in pairs[0][0].instruments)   # notes outside 21..108


def test_build_problems_raises_what_the_host_scorer_raises():
    ref, est = M.synthetic_midi(4, zero_length=True)
    with pytest.raises(ValueError) as host:
        evaluate.mt3_program_aware_note_scores(ref, est, "flat")
    with pytest.raises(ValueError) as mine:
        _host_scores([(ref, est)])
    assert str(mine.value) == str(host.value) == "all reference interval durations must be strictly positive"
    # the agnostic scores drop a zero-length note instead
    want = {k: v for k, v in evaluate.compute_transcription_metrics(ref, est).items() if "overlap" not in k}
    assert _host_scores([(ref, est)], ("onoff", "on"))[0] == want
    bad = M.midi([(0, False, [(-0.5, 0.5, 60)])])
    for pair, name in (((bad, est), "reference"), ((ref, bad), "estimated")):
        with pytest.raises(ValueError) as host:
            evaluate.compute_transcription_metrics(*pair)
        with pytest.raises(ValueError) as mine:
            _host_scores([pair], ("onoff", "on"))
        assert str(mine.value) == str(host.value) == f"negative {name} interval time"
    with pytest.raises(ValueError):
        scoring.build_problems(_notes_of([ref]), _notes_of([est, est]))


def test_abi_declares_the_matcher_and_refuses_bad_arguments():
    names = lib.header_symbols()
    for name in ("mrmt3_note_match_workspace_bytes", "mrmt3_note_match_fwd", "mrmt3_note_match_launches"):
        assert name in names
    so = lib.load()
    assert so.mrmt3_note_match_workspace_bytes(10, 20) == (4 * 20 + 2 * 10) * 4
    assert so.mrmt3_note_match_workspace_bytes(0, 0) == 0 and so.mrmt3_note_match_workspace_bytes(-1, 5) == 0
    before = lib.note_match_launches()
    buf = (ctypes.c_int * 64)()                  # 16-byte aligned below: never read, every call is refused first
    at = (ctypes.addressof(buf) + 15) & ~15
    good = dict(ref_times=at, ref_meta=at, n_ref=1, est_times=at, est_meta=at, n_est=1, ref_idx=at, ref_first=at, est_idx=at,
                est_first=at, flags=at, n_prob=1, lo=at, hi=at, n_tables=2, onset=0.05, ratio=0.2, offset=0.05, matched=at,
                match=at, status=at, ws=at, stream=None)
    bad = [{k: None} for k in ("ref_times", "ref_meta", "est_times", "est_meta", "ref_idx", "ref_first", "est_idx", "est_first",
                                "flags", "lo", "hi", "matched", "match", "status", "ws")]
    bad += [dict(n_prob=0), dict(n_prob=-1), dict(n_tables=0), dict(onset=-0.01), dict(onset=float("nan")), dict(ratio=-1.0),
            dict(ratio=float("nan")), dict(offset=-1.0), dict(offset=float("nan")), dict(ref_meta=at + 4), dict(est_meta=at + 8),
            dict(n_ref=-1), dict(n_est=1 << 31)]
    for change in bad:
        args = dict(good, **change)
        assert so.mrmt3_note_match_fwd(*args.values()) == 1, change       # MRMT3_ERR_INVALID_ARG
        assert b"note_match_fwd" in so.mrmt3_last_error()
    assert lib.note_match_launches() == before


def test_malformed_arguments_are_value_errors():
    """The wrapper refuses what `note_frames` refuses, by the same check and before it asks for device tensors."""
    import torch
    times, meta = torch.zeros(4, 2, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.int32)
    idx, first = torch.arange(4, dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32)
    lo, hi = (torch.from_numpy(t) for t in scoring.pitch_tables())
    good = dict(ref_times=times, ref_meta=meta, est_times=times, est_meta=meta, ref_idx=idx, ref_first=first, est_idx=idx,
                est_first=first, prob_flags=torch.zeros(1, dtype=torch.int32), pitch_lo=lo, pitch_hi=hi)
    before = lib.note_match_launches()
    for change in (dict(ref_times=torch.zeros(4, 4, dtype=torch.float64)[:, ::2]), dict(est_meta=meta[:, :3]),
                   dict(ref_idx=idx.long()), dict(est_first=first[:1]), dict(ref_first=first[:1], est_first=first[:1]),
                   dict(prob_flags=torch.zeros(2, dtype=torch.int32)), dict(pitch_lo=lo[:, :127].contiguous()),
                   dict(pitch_hi=hi[:1])):
        with pytest.raises(ValueError, match="note_match"):
            lib.note_match(**{**good, **change})
    with pytest.raises(RuntimeError):                # host tensors: no CPU fallback of the kernel
        lib.note_match(**good)
    assert lib.note_match_launches() == before


def test_val_notes_options():
    import train
    stem = dict(val_root="somewhere")
    assert train.val_notes_options({}, stem) is None and train.val_notes_options({"val_notes": False}, None) is None
    assert train.val_notes_options({"val_notes": True}, stem) == 0
    assert train.val_notes_options({"val_notes": "true", "val_notes_tracks": 3}, stem) == 3
    for cfg, opts in (({"val_notes": True}, None), ({"val_notes": True}, dict(val_root=None)),
                      ({"val_notes": True, "val_notes_tracks": -1}, stem), ({"val_notes": "maybe"}, stem)):
        with pytest.raises(ValueError):
            train.val_notes_options(cfg, opts)


def test_full_mix_is_every_stem_at_gain_one():
    import _stem_mix as sm
    import train
    track = sm.synthetic_tracks(1)[0]
    mix = train.full_mix(track)
    assert mix.dtype == np.float32 and len(mix) == track.n_samples
    want = np.zeros(track.n_samples, np.float32)
    for a in track.audio:
        want[:len(a)] += a
    assert (mix == want).all()
