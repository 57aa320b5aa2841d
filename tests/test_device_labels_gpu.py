"""Device-built stem-mix labels on a real MI355X: mrmt3_label_rows_fwd against the contract's host restatement
(`mrmt3.labels.label_rows_host`, which tests/test_device_labels_cpu.py holds to the definition), then the batcher, the
loader and one training step on top of it.  Every comparison is integer equality."""
import ctypes
import dataclasses
import random

import numpy as np
import pytest
import torch

import _labels as L
import _stem_mix as sm

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -0x5a5a5a5a


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec():
    from mrmt3 import labels
    from mrmt3.tokenizer import Tokenizer
    return labels.label_codec(Tokenizer())


def _launch(tab, arrays, codec, dev, event_length=1024):
    """One launch through the C ABI with guard words around `targets` and `status`: (targets, status) as numpy."""
    from mrmt3 import lib
    keep, f0, nf, total, scale, shift = arrays
    B = len(keep)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    times, meta = up(tab.times), up(tab.meta)
    d = [up(keep.view(np.int64)), up(f0), up(nf), up(total), up(scale), up(shift)]
    tg = torch.full((B * event_length + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int64)
    st = torch.full((B + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.load().mrmt3_label_rows_fwd(
        p(times) if len(tab.meta) else None, p(meta) if len(tab.meta) else None, len(tab.meta), tab.n_stems, *(p(t) for t in d),
        B, codec.pitch_base, codec.velocity_base, codec.tie_token, codec.program_base, codec.drum_base, codec.max_shift_steps,
        codec.steps_per_second, codec.sample_rate, codec.hop, event_length, codec.num_special_tokens,
        ctypes.c_void_p(tg.data_ptr() + 8 * GUARD), ctypes.c_void_p(st.data_ptr() + 4 * GUARD),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.load().mrmt3_last_error()
    tg, st = tg.cpu().numpy(), st.cpu().numpy()
    for buf in (tg, st):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "a guard word was written"
    return tg[GUARD:-GUARD].reshape(B, event_length), st[GUARD:-GUARD]


def _same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]][:40].tolist(), want[bad[0]][:40].tolist())


def test_kernel_equals_the_host_restatement_on_the_fuzz(dev, codec):
    """384 rows in 8 launches: every subset, shift and window kind of the CPU fuzz, both time grids, notes confined and
    running past the end; once more at event_length 16 (truncation)."""
    from mrmt3 import labels, lib
    lib.label_launches(reset=True)
    for i, tr in enumerate(L.fuzz_tracks(2)):
        tab, arrays = labels.note_table(tr), L.row_arrays(L.fuzz_rows(tr, i))
        got, status = _launch(tab, arrays, codec, dev)
        assert not status.any(), status
        _same(got, labels.label_rows_host(tab, *arrays, codec)[0], tr.name)
        if i < 2:
            got16, status = _launch(tab, arrays, codec, dev, 16)
            assert not status.any() and (got16[:, -1] != -100).any()      # some rows are cut
            _same(got16, labels.label_rows_host(tab, *arrays, codec, 16)[0], tr.name + " at 16")
    assert lib.label_launches() == 10


def test_a_row_that_exactly_fills_event_length_gets_no_eos(dev, codec):
    from mrmt3 import labels
    tr = L.fuzz_track(5, False, False)
    tab = labels.note_table(tr)
    arrays = tuple(a[:1] for a in L.row_arrays(L.fuzz_rows(tr, 0)))
    full = labels.label_rows_host(tab, *arrays, codec)[0][0]
    n = int(np.nonzero(full == 1)[0][0])
    assert 8 < n < 1024
    for length in (n, n + 1, n - 1):
        got, status = _launch(tab, arrays, codec, dev, length)
        _same(got, labels.label_rows_host(tab, *arrays, codec, length)[0], length)
    assert _launch(tab, arrays, codec, dev, n)[0][0, -1] == full[n - 1] != 1
    assert _launch(tab, arrays, codec, dev, n + 1)[0][0, -1] == 1


def test_chunked_shifts_empty_subset_and_the_quirk(dev, codec):
    """max_shift_steps 100 at the ABI over a 2.5 s silent gap; a kept subset with no notes (and no stem at all) gives `tie`
    alone; a row behind the only note repeats the state before the last step's first event."""
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3 import labels
    from mrmt3.stems import StemTrack
    one = NoteSequence([Note(0.1, 0.5, 60, 90, 0, False, 0)], 0.5)
    late = NoteSequence([Note(0.2, 0.3, 62, 90, 5, False, 0), Note(2.8, 2.9, 62, 90, 5, False, 0)], 2.9)
    tr = StemTrack("t", ["a", "b", "c"], [np.zeros(64000, np.float32)] * 3, [one, late, NoteSequence()],
                   [(0, False), (5, False), (0, False)])
    tab = labels.note_table(tr)
    T = labels.tokenizer_frames(64000, 128)
    arrays = (np.array([2, 4, 0, 1, 3], np.uint64), np.array([0, 0, 0, 200, 0], np.int64),
              np.array([T, 256, 256, 100, T], np.int64), np.full(5, T, np.int64), np.ones(5), np.zeros(5, np.int32))
    short = dataclasses.replace(codec, max_shift_steps=100)
    got, status = _launch(tab, arrays, short, dev, 32)
    assert not status.any()
    _same(got, labels.label_rows_host(tab, *arrays, short, 32)[0], "constructions")
    p, v, pi, tie = (b + 3 for b in (codec.program_base, codec.velocity_base, codec.pitch_base, codec.tie_token))
    assert got[0, :12].tolist() == [tie, 23, p + 5, v + 1, pi + 62, 33, v, pi + 62, 103, 103, 83, v + 1]
    assert got[1, :3].tolist() == got[2, :3].tolist() == [tie, 1, -100]
    assert got[3, :5].tolist() == [p, pi + 60, tie, 1, -100]
    empty = labels.note_table(dataclasses.replace(tr, notes=[NoteSequence()] * 3))
    got, status = _launch(empty, arrays, short, dev, 32)                  # a table without notes: null pointers, n_notes 0
    assert not status.any() and (got[:, :3] == [tie, 1, -100]).all()


def test_a_row_whose_scaled_starts_tie_against_the_links_says_so(dev, codec):
    from mrmt3 import labels
    from mrmt3.batching import StemMixBatcher, StemMixPlan, CropPlan
    tr, rows = L.collapse_track()
    arrays = L.row_arrays(rows)
    got, status = _launch(labels.note_table(tr), arrays, codec, dev)
    assert status.tolist() == [labels.STATUS_ORDER]
    unshifted = arrays[:4] + (np.ones(1), np.zeros(1, np.int32))
    got, status = _launch(labels.note_table(tr), unshifted, codec, dev)  # unscaled, the links are the order
    assert not status.any()
    _same(got, labels.label_rows_host(labels.note_table(tr), *unshifted, codec)[0], "unshifted")
    # the batcher hands the row to the host path
    step, _ = L.speed(3)
    bt = StemMixBatcher(dev, mel_length=256, event_length=64, device_labels=True)
    plan = StemMixPlan(CropPlan(np.array([0], np.int64), np.array([256], np.int32), np.array([0], np.int64)),
                       np.ones((1, 2), bool), np.ones((1, 2), np.float32), 3, step)
    tg = bt.device_targets(tr, plan)[0]
    from mrmt3.batching import pad_targets
    assert bt.host_label_rows == 1 and np.array_equal(tg.cpu().numpy(), pad_targets(bt.row_targets(tr, plan), 64).numpy())


def _dense_track():
    """One pitched stem of 1100 notes inside 2 s (2200 events in one window, above the kernel's 2048) beside a sparse one."""
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.stems import StemTrack
    dense = NoteSequence([Note(0.05 + 0.0017 * i, 0.05 + 0.0017 * i + 0.03, 30 + i % 64, 90, 7, False, 0) for i in range(1100)])
    sparse = NoteSequence([Note(0.5 * i + 0.1, 0.5 * i + 0.3, 60, 90, 0, False, 0) for i in range(8)])
    for ns in (dense, sparse):
        ns.total_time = max(n.end_time for n in ns.notes)
    return StemTrack("dense", ["d", "s"], [np.zeros(16000 * 5, np.float32)] * 2, [dense, sparse], [(7, False), (0, False)])


def test_overflowing_row_says_so_and_the_batcher_rebuilds_exactly_that_row(dev, codec):
    from mrmt3 import labels, lib
    from mrmt3.batching import StemMixBatcher
    assert lib.LABEL_CAPACITY == 2048
    tr = _dense_track()
    tab = labels.note_table(tr)
    T = labels.tokenizer_frames(80000, 128)
    arrays = (np.array([3, 3, 2], np.uint64), np.array([0, 300, 0], np.int64), np.array([256, 256, 256], np.int64),
              np.full(3, T, np.int64), np.ones(3), np.zeros(3, np.int32))
    got, status = _launch(tab, arrays, codec, dev)
    assert status.tolist() == [labels.STATUS_EVENTS, 0, 0]
    _same(got[1:], labels.label_rows_host(tab, *arrays, codec)[0][1:], "rows beside the overflowing one")
    geom = dict(mel_length=256, event_length=1024, num_rows_per_batch=2, split_frame_length=300, is_deterministic=True)
    on, off = StemMixBatcher(dev, device_labels=True, **geom), StemMixBatcher(dev, **geom)
    (mel, tg), (mel0, tg0) = on.build(tr), off.build(tr)
    assert on.host_label_rows == 1 and torch.equal(tg, tg0) and torch.equal(mel, mel0)
    assert (tg0[0] != -100).all()                                        # (the overflowing row fills event_length)


@pytest.mark.parametrize("pitch_shift,deterministic", [(0, False), (4, False), (0, True)])
def test_batcher_device_labels_equal_host_labels(dev, pitch_shift, deterministic):
    """Same mel bits, same targets, same rng state afterwards; the note table counts towards the cache and leaves with
    its pool; with the option off the label kernel is never launched."""
    from mrmt3 import labels, lib
    from mrmt3.batching import StemMixBatcher, stem_pool_layout
    tracks = sm.synthetic_tracks(2)
    geom = dict(mel_length=256, event_length=256, num_rows_per_batch=2, split_frame_length=300, min_stems=1,
                pitch_shift=pitch_shift, is_deterministic=deterministic)
    pool_bytes = [stem_pool_layout([len(a) for a in t.audio], 128)[1] * 4 for t in tracks]
    on = StemMixBatcher(dev, rng=random.Random(3), device_labels=True, cache_bytes=pool_bytes[0] + 4096, **geom)
    off = StemMixBatcher(dev, rng=random.Random(3), **geom)
    lib.label_launches(reset=True)
    shifts = set()
    for visit in range(3):
        for tr in tracks:
            before = lib.label_launches()
            mel0, tg0 = off.build(tr)
            assert lib.label_launches() == before                         # off: not one launch
            plan = on.plan(tr)
            shifts.add(plan.shift)
            mel, tg = on.build(tr, plan)
            assert lib.label_launches() == before + 1                     # on: exactly one
            assert tg.dtype == torch.int64 and tg.shape == tg0.shape and torch.equal(tg, tg0), (visit, tr.name)
            assert mel.dtype == mel0.dtype and torch.equal(mel, mel0)
            assert on.rng.getstate() == off.rng.getstate()
            assert on.cached_tracks() == [tr.name] == list(on._notes)    # the table left with the evicted pool
            assert on.cached_bytes() == pool_bytes[tracks.index(tr)] + labels.note_table(tr).nbytes
    assert on.host_label_rows == 0 and (pitch_shift == 0 or len(shifts) > 1)


def test_batcher_with_prev_equals_row_targets_prev(dev):
    from mrmt3.batching import StemMixBatcher, pad_targets
    tracks = sm.synthetic_tracks(2)
    geom = dict(mel_length=64, event_length=128, num_rows_per_batch=2, split_frame_length=300, pitch_shift=3)
    bt = StemMixBatcher(dev, rng=random.Random(11), device_labels=True, with_prev=True, **geom)
    host = StemMixBatcher("cpu", **geom)
    kinds = set()
    for visit in range(3):
        for tr in tracks:
            plan = bt.plan(tr)
            mel, tg, prev = bt.build(tr, plan)
            B = len(plan.crops.start_frame)
            assert mel.shape == (B, 64, 512) and tg.shape == prev.shape == (B, 128) and prev.dtype == torch.int64
            assert np.array_equal(tg.cpu().numpy(), pad_targets(host.row_targets(tr, plan), 128).numpy())
            assert np.array_equal(prev.cpu().numpy(), pad_targets(host.row_targets_prev(tr, plan), 128).numpy())
            kinds.update(bt.prev_windows(plan).tolist())
            for b in np.nonzero(~bt.prev_windows(plan))[0]:
                assert prev[b, :3].tolist() == [1134, 1, -100]            # the placeholder
    assert kinds == {True, False} and bt.host_label_rows == 0
    det = StemMixBatcher(dev, device_labels=True, with_prev=True, is_deterministic=True, **dict(geom, pitch_shift=0))
    prev = det.build(tracks[0])[2]
    assert (prev[:, :3].cpu() == torch.tensor([1134, 1, -100])).all()     # deterministic plans: always the placeholder


def test_one_trainer_step_of_a_with_prev_model_on_a_loader_triple(dev):
    import train
    from mrmt3.batching import StemMixBatcher
    from mrmt3.trainer import Trainer
    from test_train_infer_gpu import _model
    bt = StemMixBatcher(dev, mel_length=256, event_length=192, num_rows_per_batch=1, split_frame_length=600,
                        device_labels=True, with_prev=True)
    batch = next(iter(train.StemLoader(sm.synthetic_tracks(2), bt, 2, seed=5)))
    assert len(batch) == 3 and batch[0].shape == (2, 256, 512) and batch[1].shape == batch[2].shape == (2, 192)
    _, mel, tg, prev = next(train.loader_batches([batch], dev, 1, None))
    m = _model("with_prev", dev)
    trn = Trainer(m, lr=1e-3, track_grad_norm=True)
    loss = trn.train_step(mel, tg, prev).item()
    norm = trn.last_grad_norm.item()
    trn.close()
    assert np.isfinite(loss) and loss > 0 and np.isfinite(norm) and norm > 0
