"""Cross-track stem mixes and per-row pitch shifts without a GPU: the host restatement of
mrmt3_label_rows_parts_fwd against the definition, the planner, the audio tables, the arena and the options."""
import dataclasses
import random

import numpy as np
import pytest

import _cross_mix as X
import _labels as L


@pytest.fixture(scope="module")
def tokenizer():
    from mrmt3.tokenizer import Tokenizer
    return Tokenizer()


@pytest.fixture(scope="module")
def codec(tokenizer):
    from mrmt3 import labels
    return labels.label_codec(tokenizer)


def _same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]][:40].tolist(), want[bad[0]][:40].tolist())


def test_restatement_equals_the_definition_on_the_fuzz(tokenizer, codec):
    """1024 rows of 1-4 parts: every row is compared (a virtual track without a note against `tie` alone), no status."""
    from mrmt3 import labels
    seen_parts, seen_delays, seen_shifts, n_rows = set(), set(), set(), 0
    for seed in range(4):
        tracks = X.part_tracks(seed)
        arena, where = X.arena_of(tracks)
        rows = X.fuzz_rows(tracks, seed, 64)
        got, status = labels.label_rows_parts_host(arena, *X.row_arrays(rows, where), codec)
        assert not status.any(), status
        _same(got, X.definition_rows(tokenizer, rows), seed)
        n_rows += len(rows)
        for r in rows:
            seen_parts.add(len(r.parts))
            seen_delays.update(p.delay_frames for p in r.parts)
            seen_shifts.update(p.shift for p in r.parts)
    assert n_rows >= 1000 and seen_parts == {1, 2, 3, 4} and seen_delays == set(X.DELAYS) and seen_shifts == {0, 3, -5}


def test_truncated_rows_equal_the_definition(tokenizer, codec):
    from mrmt3 import labels
    tracks = X.part_tracks(1)
    arena, where = X.arena_of(tracks)
    rows = X.fuzz_rows(tracks, 9, 8)
    got, status = labels.label_rows_parts_host(arena, *X.row_arrays(rows, where), codec, 16)
    _same(got, X.definition_rows(tokenizer, rows, 16), "at 16")
    assert (got[:, -1] != -100).any() and not status.any()


def test_one_part_without_delay_is_label_rows_host(codec):
    from mrmt3 import labels
    for i, tr in enumerate(L.fuzz_tracks(1)):
        tab = labels.note_table(tr)
        keep, f0, nf, total, scale, shift = L.row_arrays(L.fuzz_rows(tr, i))
        B = len(keep)
        col = lambda a: np.ascontiguousarray(a.reshape(B, 1))
        got, status = labels.label_rows_parts_host(
            tab, np.zeros((B, 1), np.int32), np.full((B, 1), len(tab.meta), np.int32), col(keep), np.zeros((B, 1), np.int64),
            col(scale), col(shift), f0, nf, total, codec)
        assert not status.any()
        _same(got, labels.label_rows_host(tab, keep, f0, nf, total, scale, shift, codec)[0], tr.name)


def test_a_table_anywhere_in_the_arena_gives_the_same_row(codec):
    from mrmt3 import labels
    tracks = X.part_tracks(2)
    arena, where = X.arena_of(tracks)
    rows = X.windows(X.make_parts([tracks[2]], [(0, 1, 3)], [3], [0]), np.random.RandomState(0))
    alone, where1 = X.arena_of([tracks[2]])
    a = labels.label_rows_parts_host(arena, *X.row_arrays(rows, where), codec)
    b = labels.label_rows_parts_host(alone, *X.row_arrays(rows, where1), codec)
    assert where[tracks[2].name][0] > 0 and np.array_equal(a[0], b[0]) and not a[1].any() and not b[1].any()


def test_a_shared_pair_is_status_16_and_the_definition_still_yields_the_row(tokenizer, codec):
    """Parts 0 and 1 both built at position 0: program 0 and the drum stem are in both."""
    from mrmt3 import labels
    tracks = [X.part_track(3, True, False, 0), dataclasses.replace(X.part_track(4, True, False, 0), name="other")]
    arena, where = X.arena_of(tracks)
    rs = np.random.RandomState(1)
    rows = X.windows(X.make_parts(tracks, [(0, 3), (2,)], [0, 3], [0, 250]), rs)         # program 0 twice
    rows += X.windows(X.make_parts(tracks, [(0,), (3,)], [0, 0], [1, 0]), rs)           # programs 0 and 40: disjoint
    got, status = labels.label_rows_parts_host(arena, *X.row_arrays(rows, where), codec)
    assert status.tolist() == [labels.STATUS_SHARED] * 4 + [0] * 4
    _same(got, X.definition_rows(tokenizer, rows), "shared pair")


# ---- the planner -------------------------------------------------------------------------------------------------------

class LogRng:
    """random.Random that writes down every draw it hands out."""

    def __init__(self, seed):
        self.r, self.log, self.values = random.Random(seed), [], {}

    def randint(self, a, b):
        self.log.append(("randint", a, b))
        return self.r.randint(a, b)

    def random(self):
        self.log.append(("random",))
        self.values[len(self.log) - 1] = v = self.r.random()
        return v

    def uniform(self, a, b):
        self.log.append(("uniform", a, b))
        return self.r.uniform(a, b)


GEOM = dict(mel_length=32, event_length=64, num_rows_per_batch=4, split_frame_length=90)


def _batcher(rng=None, **kw):
    from mrmt3.batching import StemMixBatcher
    return StemMixBatcher("cpu", rng=rng, device_labels=True, **dict(GEOM, **kw))


def _tracks():
    return X.part_tracks(3)


def _same_plan(a, b):
    return (all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("part", "shift", "step", "start", "chunk_start", "n_frames"))
            and all(np.array_equal(x, y) for x, y in zip(a.keep + a.gain, b.keep + b.gain)))


def test_plan_cross_is_a_function_of_the_rng():
    tr = _tracks()
    kw = dict(cross_track=True, per_row_shift=True, pitch_shift=5, cross_prob=0.7)
    a = _batcher(random.Random(5), **kw).plan_cross(tr[0], tr[1:])
    b = _batcher(random.Random(5), **kw).plan_cross(tr[0], tr[1:])
    c = _batcher(random.Random(6), **kw).plan_cross(tr[0], tr[1:])
    assert _same_plan(a, b) and not _same_plan(a, c)
    assert a.part[:, 1:].any() and not a.part[:, 1:].all() and len(set(a.shift.reshape(-1).tolist())) > 2


def test_plan_cross_draws_in_the_documented_order():
    from mrmt3.batching import plan_stem_mix
    from mrmt3.stems import shift_range
    tr = _tracks()
    S = 5
    bt = _batcher(LogRng(11), cross_track=True, per_row_shift=True, pitch_shift=S, cross_prob=0.6)
    plan = bt.plan_cross(tr[0], tr[1:])
    ref = LogRng(11)
    base = plan_stem_mix(bt.n_frames(tr[0]), 4, GEOM["mel_length"], GEOM["num_rows_per_batch"], GEOM["split_frame_length"],
                         0.75, 1, 6.0, False, ref)
    log = bt.rng.log
    assert log[:len(ref.log)] == ref.log and np.array_equal(plan.base.keep, base.keep)     # 1: plan_stem_mix, unshifted
    at = len(ref.log)
    B = len(plan.n_frames)
    assert B == 4
    for b in range(B):
        assert log[at] == ("randint", -S, S)                                               # (a)
        at += 1
        lo, hi = shift_range(tr[0])
        assert lo <= plan.shift[b, 0] <= hi
        for t in (1, 2, 3):
            assert log[at] == ("random",)                                                   # (b) takes part?
            at += 1
            took = bt.rng.values[at - 1] < 0.6
            borrowed = int(plan.keep[t][b].sum())
            if not took:
                assert not plan.part[b, t]
                continue
            assert log[at] == ("randint", -S, S)                                            # its shift
            assert log[at + 1][0] == "randint" and log[at + 1][1] == 0                      # its start
            if plan.part[b, t]:
                frames = bt.n_frames(tr[t], int(plan.step[b, t]))
                assert log[at + 1] == ("randint", 0, max(0, frames - GEOM["mel_length"]))
                assert 0 <= plan.start[b, t] <= log[at + 1][2]
            assert log[at + 2:at + 6] == [("random",)] * 4                                  # one per stem, kept or not
            assert [bt.rng.values[at + 2 + s] < 0.75 for s in range(4)] == plan.keep[t][b].tolist()   # (pairs are disjoint)
            assert log[at + 6:at + 6 + borrowed] == [("uniform", -6.0, 6.0)] * borrowed     # one per borrowed stem
            at += 6 + borrowed
            assert plan.part[b, t] == (borrowed > 0)
    assert at == len(log)


def test_plan_cross_without_partners_and_shifts_is_plan():
    tr = _tracks()
    a = _batcher(random.Random(2), cross_track=True).plan_cross(tr[0])
    b = _batcher(random.Random(2)).plan(tr[0])
    assert np.array_equal(a.start[:, 0], b.crops.start_frame) and np.array_equal(a.n_frames, b.crops.valid_frames)
    assert np.array_equal(a.chunk_start, b.crops.chunk_start) and np.array_equal(a.keep[0], b.keep)
    assert np.array_equal(a.gain[0], b.gain) and not a.any_shift and a.part.shape[1] == 1
    det = _batcher(random.Random(2), cross_track=True, per_row_shift=True, pitch_shift=4, is_deterministic=True)
    d = det.plan_cross(tr[0], tr[1:])                                                       # partners and shifts ignored
    p = _batcher(is_deterministic=True).plan(tr[0])
    assert d.part.shape[1] == 1 and not d.any_shift and np.array_equal(d.start[:, 0], p.crops.start_frame)
    assert d.keep[0].all() and (d.gain[0] == 1).all()


def test_no_row_keeps_a_pair_in_two_parts_and_sources_are_bounded():
    """Partners built at the SAME part position share every pair with the visited track: nothing of them is borrowed but
    what the visited track dropped."""
    tr = [X.part_track(k, True, False, 0) for k in range(3)]
    bt = _batcher(random.Random(4), cross_track=True, cross_prob=1.0, keep_prob=0.5)
    seen = 0
    for _ in range(20):
        plan = bt.plan_cross(tr[0], tr[1:])
        for b in range(len(plan.n_frames)):
            pairs = [{t.programs[s] for s in np.nonzero(plan.keep[i][b])[0]} for i, t in enumerate(plan.tracks) if plan.part[b, i]]
            for i in range(len(pairs)):
                for j in range(i):
                    assert not pairs[i] & pairs[j]
            seen += len(pairs) > 1
    assert seen > 5
    from mrmt3.stems import StemTrack
    wide = lambda name: StemTrack(name, ["s"] * 33, [np.zeros(4000, np.float32)] * 33, tr[0].notes[:1] * 33, [(0, False)] * 33)
    with pytest.raises(ValueError, match="64 sources"):
        bt.plan_cross(wide("a"), [wide("b")])
    with pytest.raises(ValueError, match="at most 4 parts"):
        bt.plan_cross(tr[0], [tr[1]] * 4)
    with pytest.raises(ValueError, match="cross_track"):
        _batcher(per_row_shift=True, pitch_shift=2).plan_cross(tr[0], tr[1:])
    for kw in (dict(cross_track=True), dict(per_row_shift=True)):
        with pytest.raises(ValueError, match="device_labels"):
            from mrmt3.batching import StemMixBatcher
            StemMixBatcher("cpu", **kw)


# ---- the audio tables --------------------------------------------------------------------------------------------------

def _nan_pool(bt, plan, rs):
    """A pool in which the plan's tracks lie in odd places with NaN between the slots and between the stems (the padding
    of a stem to its whole hop): (pool, bases)."""
    from mrmt3.batching import stem_pool_layout
    hop = 128
    pieces, bases, at = [], [], 0
    for t in reversed(plan.tracks):                      # not the order of the plan
        gap = hop * int(rs.randint(1, 4))
        pieces.append(np.full(gap, np.nan, np.float32))
        at += gap
        lengths = bt.lengths(t)
        offsets, total = stem_pool_layout(lengths, hop)
        slot = np.full(total, np.nan, np.float32)
        for off, n in zip(offsets, lengths):
            slot[off:off + n] = rs.uniform(-1, 1, n).astype(np.float32)
        pieces.append(slot)
        bases.append(at)
        at += total
    pieces.append(np.full(hop, np.nan, np.float32))
    return np.concatenate(pieces), np.array(bases[::-1], np.int64)


@pytest.mark.parametrize("shifted", [False, True])
def test_cross_tables_pass_the_checkers_and_stay_inside_their_stems(shifted):
    import _resample as rsm
    import _stem_mix as sm
    from mrmt3.batching import stem_pool_layout
    from mrmt3.resample import resample_filter, stack_filters
    from fractions import Fraction
    tr = _tracks()
    bt = _batcher(random.Random(8), cross_track=True, per_row_shift=shifted, pitch_shift=4 if shifted else 0, cross_prob=0.8,
                  mel_length=8)
    plan = bt.plan_cross(tr[0], tr[1:])
    assert plan.any_shift == shifted and plan.part[:, 1:].any()
    pool, bases = _nan_pool(bt, plan, np.random.RandomState(0))
    tabs = bt.cross_tables(plan, bases, len(pool))                                          # (the checkers run inside)
    stems = set()
    for t, base in zip(plan.tracks, bases):
        lengths = bt.lengths(t)
        stems |= {(int(base + o), int(base + o + n)) for o, n in zip(stem_pool_layout(lengths, 128)[0], lengths)}
    n = 8 * 128
    if shifted:
        pos, begin, end, step, gain, filt, valid, steps = tabs
        on = gain != 0
        assert on.any() and all((int(b), int(e)) in stems for b, e in zip(begin[on], end[on]))
        assert ((pos[on] >> 32) >= begin[on]).all() and ((pos[on] >> 32) < end[on]).all()
        assert ((filt == -1) == (step == 1 << 32))[on].all() and gain.shape[1] == 16 <= 64
        f = stack_filters([resample_filter(Fraction(s, 1 << 32)) for s in steps])
        rows = rsm.resample_rows(pool, pos, begin, end, step, gain, filt, n, f, valid)
    else:
        start, end, gain = tabs
        on = gain != 0
        assert on.any() and gain.shape[1] == 16
        for b, k in zip(*np.nonzero(on)):
            mine = [s for s in stems if s[1] == end[b, k]]
            assert len(mine) == 1 and mine[0][0] <= start[b, k] * 128 < mine[0][1]
        rows = sm.mix_rows(pool, start * 128, end, gain, n, 128, plan.n_frames)
    assert np.isfinite(rows).all() and np.abs(rows).max() > 0                               # not one NaN was read


# ---- the arena ---------------------------------------------------------------------------------------------------------

def _no_overlap(arena):
    for which in (0, 1):
        spans = sorted(s[which] for s in arena.slots.values())
        assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert all(0 <= off and off + n <= arena.capacity[which] for off, n in spans)


def test_arena_slots_eviction_order_and_tracks_in_use():
    from mrmt3.batching import TrackArena
    ar = TrackArena(1000, 100)
    assert ar.place("a", 400, 10) == [] and ar.place("b", 300, 10) == [] and ar.place("c", 300, 10) == []
    _no_overlap(ar)
    ar.touch("a")                                                    # least recent first: b, c, a
    assert ar.place("d", 500, 10) == ["b", "c"] and list(ar.slots) == ["a", "d"]
    _no_overlap(ar)
    assert ar.place("e", 100, 85, in_use=("a", "e")) == ["d"]        # the note arena is full too soon; a is in use
    _no_overlap(ar)
    with pytest.raises(ValueError, match="does not fit"):
        ar.place("f", 700, 1, in_use=("a", "f"))
    with pytest.raises(ValueError, match="does not fit"):
        TrackArena(10, 10).place("g", 11, 1)
    rs = np.random.RandomState(0)
    ar = TrackArena(4096, 256)
    for k in range(200):                                             # a long random run never overlaps
        ar.place("t%d" % k, 128 * int(rs.randint(1, 12)), int(rs.randint(1, 60)))
        if rs.randint(2) and len(ar.slots) > 1:
            ar.touch(list(ar.slots)[0])
        _no_overlap(ar)


# ---- train.py ----------------------------------------------------------------------------------------------------------

def test_stem_options_validate_the_cross_keys(tmp_path):
    from mrmt3 import hydra_lite
    from test_config_cpu import MODEL, TOP
    import train
    (tmp_path / "model").mkdir()
    (tmp_path / "dataset").mkdir()
    (tmp_path / "config.yaml").write_text(TOP)
    (tmp_path / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    fmt = lambda v: str(v).lower() if isinstance(v, bool) else str(v)
    opt = lambda **kw: train.stem_options(hydra_lite.compose(str(tmp_path), "config", ["+stem_root=/d"] + [
        "+%s=%s" % (k, fmt(v)) for k, v in kw.items()]))
    o = opt(stem_device_labels=True, stem_cross=2, stem_cross_prob=0.25, stem_shift_per_row=True, stem_pitch_shift=3)
    assert o["cross"] == 2 and o["cross_prob"] == 0.25 and o["shift_per_row"] is True
    assert "cross" not in opt() and "shift_per_row" not in opt()
    for bad in (dict(stem_cross=4), dict(stem_cross=-1), dict(stem_cross=1.5), dict(stem_cross=True),
                dict(stem_cross_prob=1.5), dict(stem_cross_prob="x"), dict(stem_cross_prob=True), dict(stem_shift_per_row=2),
                dict(stem_shift_per_row="maybe")):
        with pytest.raises(ValueError, match=list(bad)[0]):
            opt(stem_device_labels=True, **bad)
    for needs in (dict(stem_cross=1), dict(stem_shift_per_row=True)):
        with pytest.raises(ValueError, match="stem_device_labels"):
            opt(**needs)
    with pytest.raises(ValueError, match="stem_shift_per_row"):
        opt(stem_device_labels=True, stem_cross=1, stem_pitch_shift=2)


def test_loader_partners_are_a_function_of_the_shard():
    import train
    tr = [X.part_track(k, True, False, k % 4) for k in range(5)]
    ld = train.StemLoader(tr, _batcher(cross_track=True), 1, seed=3, partners=2)
    shard = ld.shard()
    for j in range(len(shard)):
        ps = ld.partners_of(shard, j)
        assert [p.name for p in ps] == [tr[shard[(j + k) % 5]].name for k in (1, 2)] and tr[shard[j]] not in ps
    two = train.StemLoader(tr[:2], _batcher(cross_track=True), 1, seed=3, partners=3)
    assert [len(two.partners_of(two.shard(), j)) for j in range(2)] == [1, 1]


def test_library_has_the_entry():
    import ctypes
    from mrmt3 import labels, lib
    so = ctypes.CDLL(lib.LIB_PATH)
    assert so.mrmt3_version() >= 129 and lib.MIN_VERSION >= 129 and callable(lib.label_rows_parts)
    assert "mrmt3_label_rows_parts_fwd" in lib.header_symbols() and lib.LABEL_MAX_PARTS == labels.MAX_PARTS == 4


def test_the_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    from mrmt3 import lib
    so = lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) & ~15
    lib.label_launches(reset=True)
    names = ("note_times", "note_meta", "n_notes", "n_parts", "note_first", "note_count", "keep", "delay_frames", "scale",
             "shift", "start_frame", "n_frames", "total_frames", "batch", "pitch_base", "velocity_base", "tie_token",
             "program_base", "drum_base", "max_shift_steps", "steps_per_second", "sample_rate", "hop", "event_length",
             "num_special_tokens", "targets", "status", "stream")
    good = [a, a, 4, 2, a, a, a, a, a, a, a, a, a, 3, 1001, 1129, 1131, 1132, 1260, 1000, 100, 16000, 128, 64, 3, a, a, None]
    assert len(names) == len(good)
    cases = [(n, None, b"null") for n in names if good[names.index(n)] == a]
    cases += [("n_parts", 0, b"n_parts"), ("n_parts", 5, b"n_parts"), ("batch", 0, b"batch"), ("batch", -2, b"batch"),
              ("n_notes", -1, b"null note arena"), ("event_length", 0, b"event_length"), ("max_shift_steps", 0, b"max_shift"),
              ("steps_per_second", 0, b"steps_per_second"), ("sample_rate", 0, b"sample_rate"), ("hop", 0, b"hop"),
              ("tie_token", -1, b"token bases"), ("note_meta", a + 4, b"aligned")]
    for name, val, word in cases:
        args = list(good)
        args[names.index(name)] = val
        assert so.mrmt3_label_rows_parts_fwd(*args) == 1 and word in so.mrmt3_last_error(), (name, val, so.mrmt3_last_error())
    assert lib.label_launches() == 0                                     # nothing was launched
