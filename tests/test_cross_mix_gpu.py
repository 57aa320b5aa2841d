"""Cross-track stem mixes on a real MI355X: mrmt3_label_rows_parts_fwd against its host restatement
(`mrmt3.labels.label_rows_parts_host`, which tests/test_cross_mix_cpu.py holds to the definition) and against
mrmt3_label_rows_fwd, then the audio tables, the batcher, the loader and train.py on top.  Every comparison is integer or
bit equality."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import _cross_mix as X
import _labels as L

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
def tokenizer():
    from mrmt3.tokenizer import Tokenizer
    return Tokenizer()


@pytest.fixture(scope="module")
def codec(tokenizer):
    from mrmt3 import labels
    return labels.label_codec(tokenizer)


def _launch(arena, arrays, codec, dev, event_length=1024):
    """One launch through the C ABI with guard words around `targets` and `status`: (targets, status) as numpy."""
    from mrmt3 import lib
    B, P = arrays[2].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    times, meta = up(arena.times), up(arena.meta)
    d = [up(a.view(np.int64) if a.dtype == np.uint64 else a) for a in arrays]
    tg = torch.full((B * event_length + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int64)
    st = torch.full((B + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    N = len(arena.meta)
    rc = lib.load().mrmt3_label_rows_parts_fwd(
        p(times) if N else None, p(meta) if N else None, N, P, *(p(t) for t in d), B, codec.pitch_base, codec.velocity_base,
        codec.tie_token, codec.program_base, codec.drum_base, codec.max_shift_steps, codec.steps_per_second,
        codec.sample_rate, codec.hop, event_length, codec.num_special_tokens, ctypes.c_void_p(tg.data_ptr() + 8 * GUARD),
        ctypes.c_void_p(st.data_ptr() + 4 * GUARD), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.load().mrmt3_last_error()
    tg, st = tg.cpu().numpy(), st.cpu().numpy()
    for buf in (tg, st):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "a guard word was written"
    return tg[GUARD:-GUARD].reshape(B, event_length), st[GUARD:-GUARD]


def _same(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]][:40].tolist(), want[bad[0]][:40].tolist())


def test_kernel_equals_the_host_restatement_on_the_fuzz(dev, codec):
    """384 rows of 1-4 parts in 3 launches, one more at event_length 16 (truncation); the launches are counted."""
    from mrmt3 import labels, lib
    lib.label_launches(reset=True)
    for seed in range(3):
        tracks = X.part_tracks(seed)
        arena, where = X.arena_of(tracks)
        arrays = X.row_arrays(X.fuzz_rows(tracks, 50 + seed, 32), where)
        got, status = _launch(arena, arrays, codec, dev)
        want, want_status = labels.label_rows_parts_host(arena, *arrays, codec)
        assert np.array_equal(status, want_status) and not status.any(), status
        _same(got, want, seed)
        if seed == 0:
            got16, status = _launch(arena, arrays, codec, dev, 16)
            assert not status.any() and (got16[:, -1] != -100).any()
            _same(got16, labels.label_rows_parts_host(arena, *arrays, codec, 16)[0], "at 16")
    assert lib.label_launches() == 4


def test_one_part_rows_equal_the_old_entry(dev, codec):
    """The fuzz rows of mrmt3_label_rows_fwd through the new entry, as one part without delay: the same integers."""
    from mrmt3 import labels, lib
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for i, tr in enumerate(L.fuzz_tracks(1)):
        tab = labels.note_table(tr)
        keep, f0, nf, total, scale, shift = L.row_arrays(L.fuzz_rows(tr, i))
        B = len(keep)
        old, old_status = lib.label_rows(up(tab.times), up(tab.meta), tab.n_stems, up(keep.view(np.int64)), up(f0), up(nf),
                                         up(total), up(scale), up(shift), codec)
        col = lambda a: np.ascontiguousarray(a.reshape(B, 1))
        arrays = (np.zeros((B, 1), np.int32), np.full((B, 1), len(tab.meta), np.int32), col(keep), np.zeros((B, 1), np.int64),
                  col(scale), col(shift), f0, nf, total)
        got, status = _launch(tab, arrays, codec, dev)
        assert not status.any() and not old_status.any().item()
        _same(got, old.cpu().numpy(), tr.name)


def _track(name, stems):
    """stems: [(program, is_drum, [(start, end, pitch), ...])] -> a 4 s StemTrack."""
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.stems import StemTrack
    notes = []
    for program, drum, ns in stems:
        seq = NoteSequence([Note(s, e, p, 90, program, drum, 0) for s, e, p in ns])
        seq.total_time = max([n.end_time for n in seq.notes] + [0.0])
        notes.append(seq)
    return StemTrack(name, ["s%d" % i for i in range(len(stems))], [np.zeros(64000, np.float32)] * len(stems), notes,
                     [(p, d) for p, d, _ in stems])


def test_constructions(dev, tokenizer, codec):
    """A delay that moves an event over a step boundary; part 0 as the delayed part; a shared pair; two parts that overflow
    the event capacity together and not alone; a part without notes."""
    from mrmt3 import labels
    a = _track("a", [(0, False, [(0.1049, 0.5, 60)])])
    b = _track("b", [(5, False, [(0.2, 0.3, 62)])])
    c = _track("c", [(0, False, [(1.0, 1.2, 64)])])
    dense = [_track("d%d" % k, [(7 + k, False, [(0.05 + 0.003 * i, 0.05 + 0.003 * i + 0.02, 30 + i % 64) for i in range(600)])])
             for k in range(2)]
    tracks = [a, b, c] + dense
    arena, where = X.arena_of(tracks)
    row = lambda tr, kept, shifts, delays: X.windows(X.make_parts(tr, kept, shifts, delays), np.random.RandomState(0))[0]
    rows = [row([a], [(0,)], [0], [0]), row([a], [(0,)], [0], [1]),            # 0, 1: the onset at step 10, then at step 11
            row([a, b], [(0,), (0,)], [0, 0], [250, 0]),                         # 2: part 0 is the delayed one
            row([a, c], [(0,), (0,)], [0, 3], [0, 0]),                           # 3: program 0 in both parts
            row(dense, [(0,), (0,)], [0, 0], [0, 1]),                            # 4: 2400 events together
            row(dense[:1], [(0,)], [0], [0]), row(dense[1:], [(0,)], [0], [1]),  # 5, 6: 1200 alone
            row([a, b], [(0,), (0,)], [0, 0], [0, 0])]                           # 7: part 1 loses its notes below
    arrays = X.row_arrays(rows, where)
    arrays[1][7, 1] = 0                                                          # note_count 0
    got, status = _launch(arena, arrays, codec, dev)
    want, want_status = labels.label_rows_parts_host(arena, *arrays, codec)
    assert status.tolist() == want_status.tolist() == [0, 0, 0, labels.STATUS_SHARED, labels.STATUS_EVENTS, 0, 0, 0]
    ok = status == 0
    _same(got[ok], want[ok], "constructions")
    _same(want[:7], X.definition_rows(tokenizer, rows[:7]), "the restatement itself")
    p, v, pi, tie = (x + 3 for x in (codec.program_base, codec.velocity_base, codec.pitch_base, codec.tie_token))
    assert got[0, :5].tolist() == [tie, 13, p, v + 1, pi + 60] and got[1, :5].tolist() == [tie, 14, p, v + 1, pi + 60]
    assert got[2, :9].tolist() == [tie, 23, p + 5, v + 1, pi + 62, 33, v, pi + 62, 1]      # part 0's note: 2 s later, behind the window
    assert got[7, :9].tolist() == [tie, 13, p, v + 1, pi + 60, 53, v, pi + 60, 1]           # part 0 alone


# ---- the batcher -------------------------------------------------------------------------------------------------------

HOP = 128


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def _audible(tracks, seed=0):
    """The fuzz tracks with noise for audio (theirs is silence)."""
    rs = np.random.RandomState(seed)
    return [dataclasses.replace(t, audio=[rs.uniform(-0.5, 0.5, len(a)).astype(np.float32) for a in t.audio]) for t in tracks]


def _poison(bt, tracks):
    """NaN everywhere in the audio arena but in the stems of `tracks`; returns the arena on the host."""
    from mrmt3.batching import stem_pool_layout
    where, audio = bt._arena[0], bt._arena[1]
    keep = torch.zeros(audio.numel(), dtype=torch.bool)
    for t in tracks:
        base = where.slots[t.name][0][0]
        lengths = bt.lengths(t)
        for off, n in zip(stem_pool_layout(lengths, HOP)[0], lengths):
            keep[base + int(off):base + int(off) + n] = True
    audio[~keep.to(audio.device)] = float("nan")
    return audio.cpu().numpy()


@pytest.mark.parametrize("shifted", [False, True])
def test_rows_from_the_cross_tables_over_the_arena_equal_the_restatement(dev, shifted):
    import random
    import _resample as rsm
    import _stem_mix as sm
    from contrib import spectrograms as sp
    from mrmt3 import lib
    from mrmt3.batching import StemMixBatcher
    tr = _audible(X.part_tracks(3))
    bt = StemMixBatcher(dev, rng=random.Random(8), device_labels=True, cross_track=True, per_row_shift=shifted,
                        pitch_shift=4 if shifted else 0, cross_prob=0.8, mel_length=64, event_length=64, num_rows_per_batch=4,
                        split_frame_length=150, cache_bytes=16 << 20)
    plan = bt.plan_cross(tr[0], tr[1:])
    assert plan.any_shift == shifted and plan.part[:, 1:].any() and len(plan.n_frames) >= 2
    pool, bases = bt._resident(plan)[:2]
    assert all(bt.pool(t).numel() == sum(-(-n // HOP) * HOP for n in bt.lengths(t)) for t in tr)
    host = _poison(bt, tr)
    assert np.isnan(host).any()
    tabs = bt.cross_tables(plan, bases, pool.numel())
    n = 64 * HOP
    vf = torch.from_numpy(plan.n_frames.astype(np.int32)).to(dev)
    if shifted:
        filt = bt._filter_stack(tabs[7])
        want = rsm.resample_rows(host, *tabs[:6], n, filt.cpu().numpy(), tabs[6])
        got = lib.resample_mix(pool, *(torch.from_numpy(t).to(dev) for t in tabs[:6]), n, filt,
                               valid_samples=torch.from_numpy(tabs[6]).to(dev))
        assert np.array_equal(_bits(got), want.view(np.int32))
        want_mel = lib.logmel(torch.from_numpy(want).to(dev), sp.kernel_tables(bt.cfg, dev), valid_frames=vf, normalize=True)
    else:
        start, end, gain = tabs
        want = sm.mix_rows(host, start * HOP, end, gain, n, HOP, plan.n_frames)
        want_mel = sp.logmel_segments(torch.from_numpy(want).to(dev), valid_frames=vf)
    assert np.isfinite(want).all() and all(want[b].any() for b in range(len(want)))
    mel = bt.cross_mel(plan)
    assert mel.shape == (len(plan.n_frames), 64, 512) and np.array_equal(_bits(mel), _bits(want_mel))


def _definition(bt, plan, tokenizer, prev=False):
    """Every row of the plan (or every previous window) by the definition, padded."""
    from mrmt3.batching import pad_targets
    from mrmt3.stems import virtual_n_samples
    rows, out = [], []
    for b in range(len(plan.n_frames)):
        parts = bt.virtual_parts(plan, b)
        F = int(plan.start_frame[b])
        f0, nf = (F - bt.mel_length, bt.mel_length) if prev else (F, int(plan.n_frames[b]))
        rows.append(X.Row(parts, f0, nf, 0, virtual_n_samples(parts, 16000, HOP)))
    want = X.definition_rows(tokenizer, rows, bt.event_length)
    if prev:
        placeholder = pad_targets([tokenizer.row_targets_prev(None, 0, 0, bt.mel_length)], bt.event_length).numpy()[0]
        want[~bt.cross_prev_windows(plan)] = placeholder
    return want


@pytest.mark.parametrize("shifted", [False, True])
def test_build_with_partners_equals_the_definition(dev, tokenizer, shifted):
    """Targets and previous windows of every row, over several visits; one label launch per build; the mel is the one of
    the plan's own tables."""
    import random
    from mrmt3 import lib
    from mrmt3.batching import StemMixBatcher
    tr = _audible(X.part_tracks(2))
    bt = StemMixBatcher(dev, rng=random.Random(21), device_labels=True, with_prev=True, cross_track=True,
                        per_row_shift=shifted, pitch_shift=5 if shifted else 0, cross_prob=0.7, mel_length=64,
                        event_length=256, num_rows_per_batch=3, split_frame_length=200, cache_bytes=16 << 20)
    n_parts, kinds, shifts = set(), set(), set()
    for visit in range(3):
        primary, partners = tr[visit % 4], [t for t in tr if t is not tr[visit % 4]][:2 + visit % 2]
        plan = bt.plan_cross(primary, partners)
        before = lib.label_launches()
        mel, tg, prev = bt.build(primary, plan)
        assert lib.label_launches() == before + 1
        B = len(plan.n_frames)
        assert mel.shape == (B, 64, 512) and tg.shape == prev.shape == (B, 256) and bool(torch.isfinite(mel).all())
        _same(tg.cpu().numpy(), _definition(bt, plan, tokenizer), ("targets", visit))
        _same(prev.cpu().numpy(), _definition(bt, plan, tokenizer, prev=True), ("targets_prev", visit))
        assert np.array_equal(_bits(mel), _bits(bt.cross_mel(plan)))
        n_parts.update(plan.part.sum(axis=1).tolist())
        kinds.update(bt.cross_prev_windows(plan).tolist())
        shifts.update(plan.shift[plan.part].tolist())
    assert (len(shifts) > 2) == shifted and max(n_parts) >= 2 and kinds == {True, False} and bt.host_label_rows == 0
    mel, tg, prev = bt.build(tr[0], tr[1:3])                                 # partners in the plan's place
    assert mel.shape[1:] == (64, 512) and tg.shape == prev.shape


def test_reported_rows_are_rebuilt_and_only_they(dev, tokenizer):
    """A plan by hand: row 0 shares program 0 between two parts (status 16), row 1 overflows the event capacity over three
    parts, row 2 is in order."""
    from mrmt3.batching import CrossMixPlan, StemMixBatcher
    a = _track("a", [(0, False, [(0.1049, 0.5, 60)])])
    c = _track("c", [(0, False, [(1.0, 1.2, 64)])])
    dense = [_track("d%d" % k, [(7 + k, False, [(0.05 + 0.003 * i, 0.05 + 0.003 * i + 0.02, 30 + i % 64) for i in range(600)])])
             for k in range(2)]
    tracks = [a, c] + dense
    B, T = 3, 4
    part = np.array([[1, 1, 0, 0], [1, 0, 1, 1], [1, 0, 1, 0]], bool)
    plan = CrossMixPlan(tracks, None, part, [part[:, t:t + 1].copy() for t in range(T)],
                        [part[:, t:t + 1].astype(np.float32) for t in range(T)], np.zeros((B, T), np.int32),
                        np.full((B, T), 1 << 32, np.int64), np.array([[0, 0, 0, 0], [1, 0, 0, 1], [300, 0, 0, 0]], np.int64),
                        np.zeros(B, np.int64), np.full(B, 256, np.int32))
    bt = StemMixBatcher(dev, device_labels=True, with_prev=True, cross_track=True, mel_length=256, event_length=1024,
                        cache_bytes=8 << 20)
    rebuilt = []
    host_row = bt.cross_host_row
    bt.cross_host_row = lambda plan, b, prev=False: (rebuilt.append((b, prev)), host_row(plan, b, prev))[1]
    mel, tg, prev = bt.build(tracks[0], plan)
    assert sorted(rebuilt) == [(0, False), (1, False)] and bt.host_label_rows == 2
    _same(tg.cpu().numpy(), _definition(bt, plan, tokenizer), "targets")
    _same(prev.cpu().numpy(), _definition(bt, plan, tokenizer, prev=True), "targets_prev")
    assert bt.cross_prev_windows(plan).tolist() == [False, False, True] and (tg[1] != -100).all()


def test_eviction_and_a_second_upload_give_the_same_bits(dev):
    import random
    from mrmt3.batching import StemMixBatcher, stem_pool_layout
    tr = sorted(_audible(X.part_tracks(1)), key=lambda t: sum(len(x) for x in t.audio))
    tr = [tr[3], tr[0], tr[1], tr[2]]                                        # the pairs: (longest, shortest), (the two between)
    tot = [stem_pool_layout([len(x) for x in t.audio], HOP)[1] for t in tr]
    cap = max(tot[0] + tot[1], tot[2] + tot[3]) + HOP
    assert cap < tot[0] + tot[1] + min(tot[2], tot[3])                       # the second pair cannot lie beside the first
    bt = StemMixBatcher(dev, rng=random.Random(4), device_labels=True, cross_track=True, per_row_shift=True, pitch_shift=3,
                        cross_prob=1.0, mel_length=64, event_length=128, num_rows_per_batch=2, split_frame_length=150,
                        cache_bytes=-(-4 * cap * 32 // 31) + 64)
    assert bt.cached_bytes() == 0
    plan = bt.plan_cross(tr[0], tr[1:2])
    first = bt.build(tr[0], plan)
    assert bt.uploads == 2 and bt.cached_tracks() == [tr[0].name, tr[1].name]
    from mrmt3 import labels
    assert bt.cached_bytes() == 4 * (tot[0] + tot[1]) + sum(labels.note_table(t).nbytes for t in tr[:2])
    bt.build(tr[2], tr[3:])
    assert bt.uploads == 4 and tr[2].name in bt.cached_tracks() and tr[3].name in bt.cached_tracks()
    assert not {tr[0].name, tr[1].name} <= set(bt.cached_tracks())           # someone left
    spans = sorted(s[0] for s in bt._arena[0].slots.values())
    assert all(x[0] + x[1] <= y[0] for x, y in zip(spans, spans[1:]))
    again = bt.build(tr[0], plan)
    assert bt.uploads > 4 and all(torch.equal(x, y) for x, y in zip(first, again))
    with pytest.raises(ValueError, match="does not fit"):
        StemMixBatcher(dev, device_labels=True, cross_track=True, cache_bytes=4 * tot[0]).pool(tr[0])


def test_one_trainer_step_of_a_with_prev_model_on_a_cross_track_triple(dev):
    import _stem_mix as sm
    import train
    from mrmt3.batching import StemMixBatcher
    from mrmt3.trainer import Trainer
    from test_train_infer_gpu import _model
    bt = StemMixBatcher(dev, mel_length=256, event_length=192, num_rows_per_batch=1, split_frame_length=600,
                        device_labels=True, with_prev=True, cross_track=True, cross_prob=1.0, per_row_shift=True, pitch_shift=2)
    batch = next(iter(train.StemLoader(sm.synthetic_tracks(3), bt, 2, seed=5, partners=1)))
    assert len(batch) == 3 and batch[0].shape == (2, 256, 512) and batch[1].shape == batch[2].shape == (2, 192)
    _, mel, tg, prev = next(train.loader_batches([batch], dev, 1, None))
    m = _model("with_prev", dev)
    trn = Trainer(m, lr=1e-3, track_grad_norm=True)
    loss = trn.train_step(mel, tg, prev).item()
    norm = trn.last_grad_norm.item()
    trn.close()
    assert np.isfinite(loss) and loss > 0 and np.isfinite(norm) and norm > 0


def test_train_py_trains_on_cross_track_rows(dev, tmp_path):
    import os
    import subprocess
    import sys
    import _stem_mix as sm
    from test_config_cpu import MODEL
    top = """
num_epochs: 1
model_type: ${hydra:runtime.choices.model}
dataset_type: ${hydra:runtime.choices.dataset}
seed: 365
path:
event_length: 128
mel_length: 256
num_rows_per_batch: 2
split_frame_length: 300
optim:
  lr: 2e-4
  warmup_steps: 10
  num_epochs: ${num_epochs}
  num_steps_per_epoch: 100
  min_lr: 1e-4
trainer:
  log_every_n_steps: 1
dataloader:
  train:
    batch_size: 1
defaults:
  - model: MT3Net
  - dataset: Slakh
"""
    (tmp_path / "cfg" / "model").mkdir(parents=True)
    (tmp_path / "cfg" / "dataset").mkdir()
    (tmp_path / "cfg" / "config.yaml").write_text(top)
    (tmp_path / "cfg" / "model" / "MT3Net.yaml").write_text(MODEL % ("mt3_net.MT3Net", ""))
    (tmp_path / "cfg" / "dataset" / "Slakh.yaml").write_text("train:\n  mel_length: ${mel_length}\n")
    root = sm.write_tracks(tmp_path / "stems", sm.synthetic_tracks(3))
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mr-mt3_amd")
    r = subprocess.run([sys.executable, os.path.join(pkg, "train.py"), "--config-dir", str(tmp_path / "cfg"), "--config-name",
                        "config", f"+stem_root={root}", "+stem_device_labels=true", "+stem_cross=1", "+stem_shift_per_row=true",
                        "+stem_pitch_shift=2", "+max_steps=2", f"+output_dir={tmp_path / 'out'}"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert any(l.startswith("step 0 train_loss ") for l in lines) and any(l.startswith("step 1 train_loss ") for l in lines), r.stdout
    launches = [l for l in lines if l.startswith("label_launches ")]
    assert launches and int(launches[-1].split()[1]) >= 2, r.stdout
