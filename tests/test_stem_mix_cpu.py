"""Stem-mix training batches without a GPU: the contract's numpy restatement (tests/_stem_mix.py) pinned from two sides,
the stem folder round trip, the row plan (determinism, documented draw order, the deterministic form, min_stems, every
validation error), the targets against their definition, the C entry point's argument checks, and train.py's options."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import _stem_mix as sm

HOP = 128


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def test_mix_rows_with_one_source_at_gain_one_is_the_slice():
    rs = np.random.RandomState(0)
    pool = rs.uniform(-1, 1, 5000).astype(np.float32)
    start, end = np.array([[100], [4000], [4999]]), np.array([[5000], [4500], [5000]])
    rows = sm.mix_rows(pool, start, end, np.ones((3, 1), np.float32), 700, HOP)
    assert rows.dtype == np.float32 and rows.shape == (3, 700)
    assert np.array_equal(rows[0], pool[100:800])
    assert np.array_equal(rows[1, :500], pool[4000:4500]) and not rows[1, 500:].any()       # the stem's end, not the pool's
    assert rows[2, 0] == pool[4999] and not rows[2, 1:].any()
    vf = np.array([2, 0, 5], np.int32)                                                       # zero from valid_frames * hop on
    rows = sm.mix_rows(pool, start, end, np.ones((3, 1), np.float32), 700, HOP, vf)
    assert np.array_equal(rows[0, :256], pool[100:356]) and not rows[0, 256:].any() and not rows[1].any()


@pytest.mark.parametrize("n_src", [1, 2, 5, 64])
def test_mix_rows_lies_within_the_f32_bound_of_the_float64_sum(n_src):
    """|f32 sequential sum - float64 sum| <= n_src * 2^-24 * sum_k |g_k s_k| per sample: one rounding per product and
    one per addition, each at most 2^-24 relative of a partial sum that sum_k |g_k s_k| bounds."""
    c = sm.stem_case(n_src, 16 * HOP + 5, seed=3)
    rows = sm.mix_rows(c["pool"], c["start"], c["end"], c["gain"], c["n_samples"], HOP, c["valid_frames"])
    ref, mag = sm.mix_rows_f64(c["pool"], c["start"], c["end"], c["gain"], c["n_samples"], HOP, c["valid_frames"])
    assert np.isfinite(rows).all(), "a NaN gap was read"
    assert (np.abs(rows.astype(np.float64) - ref) <= n_src * 2.0 ** -24 * mag).all()
    assert rows[0].any() and not rows[2, 1:].any() and rows[2, 0] != 0                       # row 2: silent past sample 0
    assert not rows[1, int(c["valid_frames"][1]) * HOP:].any()


def test_mix_rows_clamps_like_the_contract():
    pool = np.arange(1, 101, dtype=np.float32)
    start = np.array([[90, -5, 50, 200, 10]])
    end = np.array([[400, 60, 50, 300, 20]])          # end past the pool; start < 0; start == end; start past the pool; plain
    gain = np.array([[1, 1, 1, 1, 2]], np.float32)
    rows = sm.mix_rows(pool, start, end, gain, 30, HOP)
    want = np.zeros(30, np.float32)
    want[:10] += pool[90:100]
    want[:10] += 2 * pool[10:20]
    assert np.array_equal(rows[0], want)
    gain[0, 4] = 0                                     # gain 0: ignored whatever it points at
    start[0, 4], end[0, 4] = -10 ** 12, 10 ** 12
    assert np.array_equal(sm.mix_rows(pool, start, end, gain, 30, HOP)[0, :10], pool[90:100])


# ---- folder round trip --------------------------------------------------------------------------------------------------------

def test_stem_folder_round_trip(tmp_path):
    from contrib import audio_io
    from mrmt3 import stems
    src = sm.synthetic_tracks(2)
    root = sm.write_tracks(tmp_path / "stems_root", src)
    got = stems.load_stem_folder(root)
    assert [os.path.basename(t.name) for t in got] == ["track00", "track01"]
    for a, b in zip(src, got):
        assert b.stem_names == a.stem_names and b.programs == a.programs and b.programs[1] == (0, True)
        assert len({len(x) for x in b.audio}) == 3 and b.n_samples == max(len(x) for x in a.audio)
        for name, xa, xb in zip(a.stem_names, a.audio, b.audio):
            back, rate = audio_io.read_wav(os.path.join(b.name, "stems", name + ".wav"))
            assert rate == 16000 and np.array_equal(xb, back)                    # what read_wav RETURNS, bit for bit
            assert len(xb) == len(xa) and 0 < np.abs(xb - xa).max() <= 0.5 / 32768 + 1e-7      # 16-bit file: not the written floats
        for na, nb in zip(a.notes, b.notes):
            ka = np.array(sorted((n.pitch, n.start_time) for n in na.notes))
            kb = np.array(sorted((n.pitch, n.start_time) for n in nb.notes))
            assert len(nb.notes) > 0 and ka.shape == kb.shape and np.array_equal(ka[:, 0], kb[:, 0])
            assert np.abs(ka[:, 1] - kb[:, 1]).max() <= 0.5 / 440 + 1e-9          # MIDI ticks: 220 per quarter at 120 bpm
            assert all((n.program, n.is_drum) == (na.notes[0].program, na.notes[0].is_drum) for n in nb.notes)
    # programs.json overrides what the MIDI file says
    with open(os.path.join(got[0].name, "programs.json"), "w") as f:
        json.dump({"s0": {"program": 40, "is_drum": False}, "s2": {"is_drum": True}}, f)
    over = stems.load_track(got[0].name)
    assert over.programs == [(40, False), (0, True), (33, True)] and all(n.program == 40 for n in over.notes[0].notes)
    # a stem without MIDI, and a wrong sample rate, name the file
    os.remove(os.path.join(got[1].name, "MIDI", "s1.mid"))
    with pytest.raises(ValueError, match="s1"):
        stems.load_stem_folder(root)
    audio_io.write_wav(os.path.join(got[0].name, "stems", "s2.wav"), src[0].audio[2], sr=22050)
    with pytest.raises(ValueError, match=r"s2\.wav.*22050"):
        stems.load_track(got[0].name)
    with pytest.raises(ValueError, match="no track"):
        stems.load_stem_folder(str(tmp_path))


def test_epoch_order_and_rank_shards():
    from mrmt3 import stems
    a, b = stems.epoch_order(11, 365, 0), stems.epoch_order(11, 365, 1)
    assert sorted(a) == list(range(11)) and a == stems.epoch_order(11, 365, 0) and a != b
    shards = [stems.rank_shard(a, r, 4) for r in range(4)]
    assert all(len(s) == 2 for s in shards) and len(set(sum(shards, []))) == 8
    assert stems.rank_shard(a, 0, 1) == a


# ---- the plan -----------------------------------------------------------------------------------------------------------------

class _Recorder:
    """A `random.Random` that writes down every draw."""

    def __init__(self, seed):
        self.r, self.log = random.Random(seed), []

    def randint(self, a, b):
        v = self.r.randint(a, b)
        self.log.append(("randint", a, b, v))
        return v

    def random(self):
        v = self.r.random()
        self.log.append(("random", v))
        return v

    def uniform(self, a, b):
        v = self.r.uniform(a, b)
        self.log.append(("uniform", a, b, v))
        return v


class _NoDraws:
    def __getattr__(self, name):
        raise AssertionError("the deterministic plan drew from the rng (%s)" % name)


GEOM = dict(mel_length=64, num_rows_per_batch=3, split_frame_length=100)


def test_plan_is_deterministic_and_draws_in_the_documented_order():
    from mrmt3.batching import plan_crops, plan_stem_mix
    n_frames, S = 777, 4
    p1 = plan_stem_mix(n_frames, S, rng=random.Random(5), **GEOM)
    p2 = plan_stem_mix(n_frames, S, rng=random.Random(5), **GEOM)
    for f in ("keep", "gain"):
        assert np.array_equal(getattr(p1, f), getattr(p2, f))
    assert np.array_equal(p1.crops.start_frame, p2.crops.start_frame)
    assert p1.gain.dtype == np.float32 and p1.keep.shape == (3, S)
    assert np.array_equal(p1.gain != 0, p1.keep)
    db = 20 * np.log10(p1.gain[p1.keep].astype(np.float64))
    assert (np.abs(db) <= 6.0 + 1e-5).all() and len(np.unique(p1.gain[p1.keep])) > 1
    # the order: plan_crops' draws first, then per row S x random(), (randint while short of min_stems), uniform per kept stem
    rec = _Recorder(9)
    p = plan_stem_mix(n_frames, S, keep_prob=0.3, min_stems=2, rng=rec, **GEOM)
    crops_only = _Recorder(9)
    c = plan_crops(n_frames, GEOM["mel_length"], GEOM["num_rows_per_batch"], GEOM["split_frame_length"], False, crops_only)
    assert rec.log[:len(crops_only.log)] == crops_only.log and len(crops_only.log) == 1 + 3
    assert np.array_equal(p.crops.start_frame, c.start_frame) and np.array_equal(p.crops.valid_frames, c.valid_frames)
    rest = rec.log[len(crops_only.log):]
    forced = 0
    for b in range(3):
        draws, rest = rest[:S], rest[S:]
        assert all(d[0] == "random" for d in draws)
        keep = [d[1] < 0.3 for d in draws]
        while sum(keep) < 2:
            d, rest = rest[0], rest[1:]
            dropped = [s for s in range(S) if not keep[s]]
            assert d[:3] == ("randint", 0, len(dropped) - 1)
            keep[dropped[d[3]]] = True
            forced += 1
        assert keep == p.keep[b].tolist()
        for s in range(S):
            if keep[s]:
                d, rest = rest[0], rest[1:]
                assert d[:3] == ("uniform", -6.0, 6.0) and p.gain[b, s] == np.float32(10.0 ** (d[3] / 20.0))
            else:
                assert p.gain[b, s] == 0
    assert rest == [] and forced > 0, "the seed should exercise the min_stems draws"


def test_deterministic_plan_draws_nothing_and_equals_plan_crops():
    from mrmt3.batching import plan_crops, plan_stem_mix
    p = plan_stem_mix(777, 3, is_deterministic=True, rng=_NoDraws(), **GEOM)
    c = plan_crops(777, GEOM["mel_length"], GEOM["num_rows_per_batch"], GEOM["split_frame_length"], True)
    for f in ("start_frame", "valid_frames", "chunk_start"):
        assert np.array_equal(getattr(p.crops, f), getattr(c, f))
    assert p.keep.all() and (p.gain == 1).all()


def test_min_stems_is_honoured():
    from mrmt3.batching import plan_stem_mix
    rng = random.Random(1)
    fewest, most = 99, 0
    for _ in range(200):
        p = plan_stem_mix(300, 5, keep_prob=0.05, min_stems=2, rng=rng, **GEOM)
        counts = p.keep.sum(1)
        fewest, most = min(fewest, int(counts.min())), max(most, int(counts.max()))
    assert fewest == 2 and most >= 2
    p = plan_stem_mix(300, 2, keep_prob=0.0, min_stems=5, rng=rng, **GEOM)        # more than there are: all of them
    assert p.keep.all()


def test_every_validation_error_fires():
    from mrmt3.batching import StemMixBatcher, check_mix_tables, mix_tables, plan_stem_mix, stem_pool_layout
    lengths = [1000, 700, 1300]
    offsets, total = stem_pool_layout(lengths, HOP)
    assert offsets.tolist() == [0, 1024, 1792] and total == 1792 + 1408
    plan = plan_stem_mix(11, 3, mel_length=4, num_rows_per_batch=2, split_frame_length=5, rng=random.Random(2), keep_prob=1.0)
    start, end, gain = mix_tables(plan, offsets, lengths, HOP)
    check_mix_tables(start, end, gain, total, HOP)
    assert end.tolist() == [[1000, 1724, 3092]] * 2 and start.dtype == np.int64 and gain.dtype == np.float32
    # a crop that begins behind a shorter stem's end: that source's table gain is 0, the plan's is not
    late = plan_stem_mix(11, 3, mel_length=4, num_rows_per_batch=2, split_frame_length=5, is_deterministic=True)
    late.crops.start_frame[:] = [6, 9]
    s2, e2, g2 = mix_tables(late, offsets, lengths, HOP)
    assert (g2 == 0).tolist() == [[False, True, False], [True, True, False]] and (late.gain == 1).all()
    check_mix_tables(s2, e2, g2, total, HOP)

    def bad(match, **kw):
        t = dict(start_frames=start.copy(), src_end=end.copy(), src_gain=gain.copy(), pool_samples=total, hop=HOP)
        for k, (idx, v) in kw.items():
            t[k][idx] = v
        with pytest.raises(ValueError, match=match):
            check_mix_tables(**t)

    bad("row 1.*not finite", src_gain=((1, 2), np.nan))
    bad("row 0.*not finite", src_gain=((0, 0), np.inf))
    bad("row 1.*outside the pool", start_frames=((1, 0), -1))
    bad("row 0.*outside the pool", src_end=((0, 2), total + 1))
    bad("row 1.*behind its stem's end", start_frames=((1, 1), 14))
    with pytest.raises(ValueError, match="share one"):
        check_mix_tables(start[:, :2], end, gain, total, HOP)
    with pytest.raises(ValueError, match="1 to 64"):
        check_mix_tables(np.zeros((1, 65), np.int64), np.ones((1, 65), np.int64), np.ones((1, 65), np.float32), 10, HOP)
    # a source with gain 0 is not looked at, by the check as by the kernel
    t = start.copy()
    t[0, 1] = -5
    g = gain.copy()
    g[0, 1] = 0
    check_mix_tables(t, end, g, total, HOP)
    for kw, match in ((dict(keep_prob=1.5), "keep_prob"), (dict(min_stems=0), "min_stems"), (dict(gain_db=-1.0), "gain_db"),
                      (dict(gain_db=float("nan")), "gain_db")):
        with pytest.raises(ValueError, match=match):
            StemMixBatcher("cpu", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StemMixBatcher("cpu").pool(sm.synthetic_tracks(1)[0])


# ---- targets ------------------------------------------------------------------------------------------------------------------

def test_row_targets_equal_their_definition_for_three_subsets():
    from mrmt3.batching import StemMixBatcher, plan_crops
    from mrmt3.stems import merged_note_sequence
    from mrmt3.tokenizer import Tokenizer
    track = sm.synthetic_tracks(1)[0]
    bt = StemMixBatcher("cpu", mel_length=64, event_length=128, num_rows_per_batch=3, split_frame_length=150,
                        is_deterministic=True)
    plan = bt.plan(track)
    assert len(plan.crops.start_frame) == 3
    subsets = [(0, 1, 2), (1,), (0, 2)]
    for b, kept in enumerate(subsets):
        plan.keep[b] = [s in kept for s in range(3)]
    for _ in range(2):                                           # (the second pass comes out of the batcher's cache)
        rows = bt.row_targets(track, plan)
        for b, kept in enumerate(subsets):
            tk = Tokenizer()
            ns = merged_note_sequence(track, kept)
            assert len(ns.notes) == sum(len(track.notes[s].notes) for s in kept) and ns.total_time == track.total_time
            want = tk.row_targets(tk.tokenize(ns, track.n_samples), int(plan.crops.start_frame[b]), int(plan.crops.valid_frames[b]))
            assert len(want) > 5 and np.array_equal(rows[b], want), (b, kept)
    assert not np.array_equal(rows[0], rows[1])
    assert all(n.instrument == 0 for s in track.notes for n in s.notes), "the track's own notes were modified"
    # the full subset is today's path on the merged track: plan_crops + Tokenizer.targets_for_crop + pad_targets
    from mrmt3.batching import pad_targets
    full = StemMixBatcher("cpu", mel_length=64, event_length=128, num_rows_per_batch=3, split_frame_length=150,
                          rng=random.Random(4), keep_prob=1.0)
    p = full.plan(track)
    tk = Tokenizer()
    crop_fn = tk.targets_for_crop(tk.tokenize(merged_note_sequence(track, (0, 1, 2)), track.n_samples))
    c = plan_crops(full.n_frames(track), 64, 3, 150, False, random.Random(4))
    assert np.array_equal(c.start_frame, p.crops.start_frame)
    want = pad_targets([crop_fn(int(s), int(v)) for s, v in zip(c.start_frame, c.valid_frames)], 128)
    assert np.array_equal(pad_targets(full.row_targets(track, p), 128).numpy(), want.numpy())


# ---- the entry point's argument checks (before any launch: no GPU needed) ----------------------------------------------------------

def test_mix_entry_point_is_declared_exported_and_checks_its_arguments():
    from mrmt3 import lib
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert lib._SIGS["mrmt3_logmel_mix_fwd"] == (ci, [vp, ll, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci, vp, vp])
    so = lib.load()
    assert so.mrmt3_version() >= 123
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, vp)                      # never dereferenced: every call below is refused before a launch

    def call(pool=p, pool_samples=100, start=p, end=p, gain=p, n_src=2, batch=1, n_samples=256, hop=128, window=p, out=p):
        return so.mrmt3_logmel_mix_fwd(pool, pool_samples, start, end, gain, n_src, batch, n_samples, hop, window, p, p, p, p,
                                       512, 4, None, 1, 0, out, None)

    for kw in (dict(pool=None), dict(start=None), dict(end=None), dict(gain=None), dict(window=None), dict(out=None)):
        assert call(**kw) == 1 and b"null" in so.mrmt3_last_error(), kw
    for n_src in (0, -1, 65):
        assert call(n_src=n_src) == 1 and b"n_src" in so.mrmt3_last_error()
    for kw in (dict(pool_samples=0), dict(batch=0), dict(n_samples=0), dict(hop=0)):
        assert call(**kw) == 1 and b"bad sizes" in so.mrmt3_last_error(), kw
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lib.logmel_mix(torch.zeros(10), torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.int64),
                       torch.ones(1, 1), 256, {})


# ---- train.py ---------------------------------------------------------------------------------------------------------------

def test_train_py_reads_the_stem_options(tmp_path):
    from mrmt3 import hydra_lite
    from test_config_cpu import MODEL, TOP
    import train
    (tmp_path / "model").mkdir()
    (tmp_path / "dataset").mkdir()
    (tmp_path / "config.yaml").write_text(TOP)
    (tmp_path / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    comp = lambda *over: hydra_lite.compose(str(tmp_path), "config", list(over))
    assert train.stem_options(comp()) is None and train.stem_options({}) is None        # without +stem_root nothing changes
    assert train.stem_options(comp("+stem_root=/data/stems")) == dict(root="/data/stems", val_root=None, keep=0.75,
                                                                      gain_db=6.0, min_stems=1)
    got = train.stem_options(comp("+stem_root=/d", "+stem_val_root=/v", "+stem_keep=0.5", "+stem_gain_db=3", "+stem_min=2"))
    assert got == dict(root="/d", val_root="/v", keep=0.5, gain_db=3.0, min_stems=2)
    for over, match in (("+stem_keep=1.5", "stem_keep"), ("+stem_gain_db=-1", "stem_gain_db"), ("+stem_min=0", "stem_min"),
                        ("+stem_keep=loud", "stem_keep")):
        with pytest.raises(ValueError, match=match):
            train.stem_options(comp("+stem_root=/d", over))
    with pytest.raises(ValueError, match="targets_prev"):
        train.stem_options(comp("+stem_root=/d"), with_prev=True)
    assert train.stem_options(comp(), with_prev=True) is None
    # the loader: len, (seed, epoch) order, disjoint rank shards — on a stub batcher, no GPU
    import torch

    class Stub:
        rng = None

        def build(self, track):
            return torch.full((2, 1), float(track)), torch.full((2, 1), int(track))

    tracks = list(range(7))
    loaders = [train.StemLoader(tracks, Stub(), 2, 365, rank=r, world=2) for r in range(2)]
    seen = []
    for ld in loaders:
        ld.set_epoch(3)
        batches = list(ld)
        assert len(ld) == len(batches) == 2 and batches[0][0].shape == (4, 1) and batches[1][0].shape == (2, 1)
        seen.append([int(v) for b in batches for v in b[1][::2, 0]])
    assert not set(seen[0]) & set(seen[1]) and len(seen[0]) == len(seen[1]) == 3
    one = train.StemLoader(tracks, Stub(), 3, 365)
    one.set_epoch(3)
    first = [int(v) for b in one for v in b[1][::2, 0]]
    assert sorted(first) == tracks and first == [int(v) for b in one for v in b[1][::2, 0]]
    one.set_epoch(4)
    assert first != [int(v) for b in one for v in b[1][::2, 0]]
    with pytest.raises(ValueError, match="sharded"):
        train.StemLoader(tracks[:1], Stub(), 1, 365, rank=0, world=2)
