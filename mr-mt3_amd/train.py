"""MI355X training driver — the build's counterpart of the reference's `train.py:21-116`.

Consumes the reference's Hydra YAML unchanged (through hydra when installed, else
`mrmt3.hydra_lite`), instantiates the task named by `cfg.model._target_`, and runs
`mrmt3.trainer.Trainer` (fused CE, hand-written backward, RCCL gradient exchange, one-launch AdamW),
one process per GPU:

    python train.py --config-dir /path/to/reference/config --config-name config_slakh_segmem \
        model=MT3NetSegMemV2WithPrev dataset=SlakhPrevAugment +synthetic=True +max_steps=100
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...      # data parallel

Data.  With `+synthetic=True` the loop runs `+max_steps` (default 10) synthetic Slakh-shaped batches (raw audio,
log-mel on the GPU).  Without it the configured `cfg.dataset.train` / `cfg.dataset.val` are instantiated and wrapped
in `torch.utils.data.DataLoader(**cfg.dataloader.*, collate_fn=cfg.dataset.collate_fn)` exactly like
`train.py:48-59`: batches are the reference's `(inputs mel, targets[, targets_prev])` tuples, the run lasts
`num_epochs` epochs (or `+max_steps`), and `val_loss` is evaluated every `trainer.check_val_every_n_epoch` epochs.
The Slakh/ComMU dataset classes themselves are the reference's `dataset/` package (librosa, note_seq, ...: out of
scope): put it on PYTHONPATH.  If it cannot be imported the driver STOPS with that message — it
never silently substitutes synthetic data.

Stem folders.  `+stem_root=DIR` trains from a folder of multi-stem tracks (`DIR/<track>/stems/<name>.wav`,
`DIR/<track>/MIDI/<name>.mid`, 16 kHz; `mrmt3/stems.py`) with no dataset package at all: every row is a random sub-mix
of a track's stems at random gains, mixed inside the log-mel kernel, labelled with the notes of the stems that sound
(`mrmt3.batching.StemMixBatcher`).  `+stem_keep=` (0.75) is the probability that a stem sounds in a row, `+stem_min=` (1)
the least number that do, `+stem_gain_db=` (6) the gain range in dB.  Row geometry is the config's (`mel_length`,
`event_length`, `num_rows_per_batch`, `split_frame_length`, `dataloader.train.batch_size` tracks per step); the track
order is a function of (seed, epoch) and the ranks take disjoint shards of it.  `+stem_val_root=DIR` gives `val_loss` on
the deterministic full mix of those tracks; `+val_notes=true` adds the note-level numbers behind it: every rank
transcribes the full mix of the first `+val_notes_tracks=K` tracks of its validation shard (0, the default: all of them) and
scores the notes on the device against the tracks' note tables, rank 0 prints `epoch N val_onset_f1 X val_onset_program_f1 Y` (and, with `+val_frames=true`, a second line `epoch N val_frame_f1 Z`)
(means over the tracks of all ranks; training weights).  `+stem_device_labels=true` builds the targets on the device, one
launch per track visit, instead of tokenising whole tracks on the host: the same targets, and `targets_prev` with them,
so a `*WithPrev` model trains from stems (without the option it is refused); the run then ends with `label_launches K`.
`+stem_cross=K` (0, at most 3; needs `+stem_device_labels=true`) gives every track visit the next K tracks of the
rank's epoch order as partners, whose stems a row borrows with probability `+stem_cross_prob=` (0.5) each;
`+stem_shift_per_row=true` draws the pitch shift per row and part instead of per visit.
`+stem_pitch_shift=N` (0) plays every track visit at 2^(k/12) times its speed, k drawn from [-N, N] semitones:
audio resampled on the device, labels transposed and rescaled in time; `+stem_native_rate=true` accepts stems at a quarter
to four times the config's rate (Slakh's 44.1 kHz) and resamples them on the device when a track is uploaded.  Validation
batches stay deterministic and unshifted.  With either on the run ends with `resample_launches K`.

Gradient accumulation: `cfg.trainer.accumulate_grad_batches` (the reference's `${grad_accum}`), else a top-level
`grad_accum`, else 1 — Lightning's semantics (mrmt3/trainer.py): the optimizer steps after every N-th batch and after an
epoch's last one; `+max_steps`, `trainer.log_every_n_steps`, the LR schedule and checkpoint steps count optimizer steps.

Gradient clipping: `trainer.gradient_clip_val` / `trainer.gradient_clip_algorithm` (norm, the default, or value) as
Lightning reads them from the same block (`+trainer.gradient_clip_val=1.0`); `+skip_nonfinite=true` drops an optimizer
step whose gradient norm is inf / NaN instead of poisoning the weights.  With either on, the step lines also carry
`grad_norm` (the norm before clipping) and the run ends with `skipped_steps K` when K > 0.

Loss options: top-level `label_smoothing` (torch.nn.CrossEntropyLoss's keyword) and `z_loss` (T5X's, MT3's recipe uses
1e-4): `+label_smoothing=0.1 +z_loss=1e-4`.  With either on, `train_loss` is the regularised objective and the step lines
carry the plain NLL next to it (`step N train_loss X nll Y`), the number that compares to `val_loss` and to other runs.

Parameter groups and EMA weights: top-level `freeze` and `no_decay`, lists of fnmatch patterns over the
state-dict keys (`+freeze='["encoder.*"]' +no_decay='["*layer_norm.weight"]'`), and `ema_decay` (`+ema_decay=0.999`).
Frozen tensors get no gradient and no update; `no_decay` tensors step with weight decay 0.  With `ema_decay`, validation
prints `val_loss` (training weights) and `val_loss_ema`, and `last_ema.pt` (the EMA weights as a bare state dict) is written
next to `last.pt`; `+export_weights=ema` makes `last.pt` itself the EMA weights.

`cfg.path` has the reference's meaning (`train.py:61-92`): a `.ckpt` resumes weights, AdamW moments and
the step counter; a `.pth` only loads weights (`strict=False`); anything else is an error.  At the end
rank 0 writes `<output_dir>/<model_type>_<dataset_type>/version_0/checkpoints/last.ckpt` (Lightning
layout) and `last.pt` (bare state dict, no `model.` prefix) like `train.py:105-116`; `+output_dir=...`
picks the root (default: the working directory, where Hydra would have put it).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from mrmt3 import hydra_lite  # noqa: E402


def synthetic_batches(cfg, rank, device, steps, with_prev):
    from mrmt3.synthetic import synth_audio, synth_labels
    B = int(cfg.dataloader.train.batch_size) * int(cfg.num_rows_per_batch)
    n = int(cfg.mel_length) * 128
    for it in range(steps):
        seed = 365 + 1000 * rank + it
        audio = torch.from_numpy(synth_audio(B, n, seed=seed)).to(device)
        labels = torch.from_numpy(synth_labels(B, int(cfg.event_length), seed=seed, full=False)).to(device)
        prev = torch.from_numpy(synth_labels(B, int(cfg.event_length), seed=seed + 7, full=False)).to(device) if with_prev else None
        yield audio, labels, prev


def real_loaders(cfg, world=1, rank=0):
    """DataLoaders over the configured datasets (train.py:48-59).  Raises with a clear message when the dataset
    package (the reference's `dataset/`, not part of this path) cannot be imported.

    With more than one rank each loader gets a `DistributedSampler` — what Lightning's DDP strategy injects into the
    reference's plain DataLoaders (`pl.Trainer(strategy="ddp...")`, config/config.yaml:45): every rank iterates a
    disjoint 1/world shard, an epoch is len(dataset)/world steps (which is what `optim.num_steps_per_epoch` counts)
    and the effective batch is world x the per-rank batch.  Returns (train_loader, val_loader, train_sampler or None)."""
    from torch.utils.data import DataLoader
    try:
        train_set = hydra_lite.instantiate(cfg.dataset.train)
        val_set = hydra_lite.instantiate(cfg.dataset.val)
        collate = hydra_lite.get_method(str(cfg.dataset.collate_fn))
    except ImportError as e:
        raise RuntimeError(
            f"cannot instantiate cfg.dataset ({cfg.dataset.train.get('_target_')}): {e}.  The dataset classes are the "
            "reference's `dataset/` package (needs librosa / note_seq): put it on PYTHONPATH, or pass +synthetic=True "
            "to run synthetic Slakh-shaped batches.") from e
    kw_t = {k: v for k, v in dict(cfg.dataloader.train).items()}
    kw_v = {k: v for k, v in dict(cfg.dataloader.val).items()}
    from torch.utils.data.distributed import DistributedSampler
    # The training order is a function of (seed, epoch) at EVERY world size — one rank included, where a plain
    # shuffle=True would draw its permutation from the global RNG and a resumed epoch would come in another order than
    # the interrupted one (samples seen twice, others never: ADVICE r4).  The batches are cut by a sampler that can drop
    # its first k batches at the index level: a resumed epoch does not decode and collate what it then throws away.
    sampler = DistributedSampler(train_set, num_replicas=world, rank=rank, shuffle=bool(kw_t.pop("shuffle", False)),
                                 seed=int(cfg.seed))
    batches = SkippingBatchSampler(sampler, int(kw_t.pop("batch_size", 1)), bool(kw_t.pop("drop_last", False)))
    if world > 1:
        kw_v.pop("shuffle", None)
        kw_v["sampler"] = DistributedSampler(val_set, num_replicas=world, rank=rank, shuffle=False)
    return (DataLoader(train_set, collate_fn=collate, batch_sampler=batches, **kw_t),
            DataLoader(val_set, collate_fn=collate, **kw_v), sampler if world > 1 else None)


class SkippingBatchSampler(torch.utils.data.BatchSampler):
    """torch's BatchSampler whose NEXT pass drops its first `skip` batches (index lists, nothing loaded); `len()` stays the
    full epoch (it is the steps-per-epoch of the resume arithmetic).  `set_epoch` goes through to the sampler."""

    def __init__(self, sampler, batch_size, drop_last):
        super().__init__(sampler, batch_size, drop_last)
        self.skip = 0

    def set_epoch(self, epoch):
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def __iter__(self):
        import itertools
        skip, self.skip = self.skip, 0
        return itertools.islice(super().__iter__(), skip, None)


def stem_options(cfg, with_prev=False):
    """None without `+stem_root`; else dict(root, val_root, keep, gain_db, min_stems) from `+stem_root=DIR`,
    `+stem_val_root=DIR`, `+stem_keep=` (default 0.75), `+stem_gain_db=` (6.0) and `+stem_min=` (1), plus `pitch_shift`
    and `native_rate` when `+stem_pitch_shift=` (semitones, default 0) / `+stem_native_rate=` (default false) are given,
    validated like the other options: a ValueError names the key; likewise `device_labels` when
    `+stem_device_labels=` (default false) is given.  Only the label kernel builds `targets_prev`: without
    `+stem_device_labels=true` a `*WithPrev` model is refused.  `+stem_cross=K` (partner tracks per visit, 0 to 3),
    `+stem_cross_prob=` (0.5, in [0, 1]) and `+stem_shift_per_row=` (false) appear as `cross`, `cross_prob` and
    `shift_per_row` when given; cross-track rows and per-row shifts need `+stem_device_labels=true`."""
    root = cfg.get("stem_root")
    if root is None or str(root).lower() in ("", "none", "null"):
        return None
    labels = cfg.get("stem_device_labels")
    if labels is not None:
        if isinstance(labels, str) and labels.lower() in ("true", "false"):
            labels = labels.lower() == "true"
        if not isinstance(labels, bool):
            raise ValueError("stem_device_labels must be true or false, got %r" % (labels,))
    if with_prev and not labels:
        raise ValueError("+stem_root builds (mel, targets) rows only: targets_prev, which the *WithPrev models train "
                         "on, is not built by the stem batcher (DESIGN 4j, out of scope) — train them through "
                         "cfg.dataset or +synthetic=True")
    val_root = cfg.get("stem_val_root")
    val_root = None if val_root is None or str(val_root).lower() in ("", "none", "null") else str(val_root)
    out = {"root": str(root), "val_root": val_root}
    for key, name, default, cast in (("stem_keep", "keep", 0.75, float), ("stem_gain_db", "gain_db", 6.0, float),
                                     ("stem_min", "min_stems", 1, int), ("stem_pitch_shift", "pitch_shift", 0, int)):
        raw = cfg.get(key)
        if raw is None and key == "stem_pitch_shift":
            continue                         # (the two newer keys appear in the result only when they are given)
        try:
            if isinstance(raw, bool) or (key == "stem_pitch_shift" and isinstance(raw, float) and raw != int(raw)):
                raise ValueError
            out[name] = default if raw is None else cast(raw)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, got %r" % (key, raw)) from None
    native = cfg.get("stem_native_rate")
    if native is not None:
        if isinstance(native, str) and native.lower() in ("true", "false"):
            native = native.lower() == "true"
        if not isinstance(native, bool):
            raise ValueError("stem_native_rate must be true or false, got %r" % (native,))
        out["native_rate"] = native
    if labels is not None:
        out["device_labels"] = labels
    cross, prob, per_row = cfg.get("stem_cross"), cfg.get("stem_cross_prob"), cfg.get("stem_shift_per_row")
    if cross is not None:
        if isinstance(cross, str) and cross.lstrip("+-").isdigit():
            cross = int(cross)
        if isinstance(cross, bool) or not isinstance(cross, int) or not 0 <= cross <= 3:
            raise ValueError("stem_cross must be an int in [0, 3] (partner tracks per visit), got %r" % (cross,))
        out["cross"] = cross
    if prob is not None:
        try:
            if isinstance(prob, bool):
                raise ValueError
            prob = float(prob)
        except (TypeError, ValueError):
            raise ValueError("stem_cross_prob must be a number, got %r" % (prob,)) from None
        if not 0.0 <= prob <= 1.0:
            raise ValueError("stem_cross_prob must be in [0, 1], got %r" % (prob,))
        out["cross_prob"] = prob
    if per_row is not None:
        if isinstance(per_row, str) and per_row.lower() in ("true", "false"):
            per_row = per_row.lower() == "true"
        if not isinstance(per_row, bool):
            raise ValueError("stem_shift_per_row must be true or false, got %r" % (per_row,))
        out["shift_per_row"] = per_row
    if (out.get("cross") or out.get("shift_per_row")) and not labels:
        raise ValueError("stem_cross and stem_shift_per_row need +stem_device_labels=true: the rows of a virtual track "
                         "are labelled by the label kernel only (DESIGN 4q)")
    if out.get("cross") and out.get("pitch_shift") and not out.get("shift_per_row"):
        raise ValueError("stem_cross with stem_pitch_shift needs +stem_shift_per_row=true: every part has its own shift "
                         "range")
    if not 0.0 <= out["keep"] <= 1.0:
        raise ValueError("stem_keep must be in [0, 1], got %r" % (out["keep"],))
    if not 0.0 <= out["gain_db"] < float("inf"):
        raise ValueError("stem_gain_db must be finite and >= 0, got %r" % (out["gain_db"],))
    if out["min_stems"] < 1:
        raise ValueError("stem_min must be at least 1, got %r" % (out["min_stems"],))
    if not 0 <= out.get("pitch_shift", 0) <= 24:
        raise ValueError("stem_pitch_shift must be an int in [0, 24] (semitones), got %r" % (out["pitch_shift"],))
    return out


class StemLoader:
    """The training (or validation) "loader" of `+stem_root`: an epoch visits this rank's shard of the tracks,
    `tracks_per_step` per batch, every track one `StemMixBatcher.build` — `(mel [rows, mel_length, 512], targets
    [rows, event_length])`, and `targets_prev` behind them when the batcher builds it, already on the device.  The track order is `mrmt3.stems.epoch_order(seed, epoch)`, the ranks
    take disjoint shards of it (`rank_shard`), and the batcher's draws restart from (seed, epoch, rank) with every
    epoch.  `shuffle=False` (validation: the deterministic full mix) keeps the folder's order.  `partners=K`
    hands every visit the next K tracks of this rank's epoch order as partner tracks, cyclic and without the visited one —
    a function of (seed, epoch, rank) like the order itself; partners are dropped from the end while the stems of all
    tracks exceed the 64 sources of a row.  Has what
    `loader_batches` asks of a loader and of a sampler: `len()`, iteration, `set_epoch`."""

    def __init__(self, tracks, batcher, tracks_per_step, seed, rank=0, world=1, shuffle=True, partners=0):
        from mrmt3 import stems
        self.n_partners = int(partners)
        self.tracks, self.batcher, self.per = tracks, batcher, max(1, int(tracks_per_step))
        self.seed, self.rank, self.world, self.shuffle, self.epoch = int(seed), rank, world, shuffle, 0
        self._stems = stems
        if not stems.rank_shard(list(range(len(tracks))), rank, world):
            raise ValueError("%d stem tracks cannot be sharded over %d ranks" % (len(tracks), world))

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def shard(self):
        n = len(self.tracks)
        order = self._stems.epoch_order(n, self.seed, self.epoch) if self.shuffle else list(range(n))
        return self._stems.rank_shard(order, self.rank, self.world)

    def __len__(self):
        return -(-len(self.shard()) // self.per)

    def partners_of(self, shard, j):
        """The partner tracks of the visit at place j of the shard."""
        ids = []
        for k in range(1, len(shard)):
            t = shard[(j + k) % len(shard)]
            if t != shard[j] and t not in ids and len(ids) < self.n_partners:
                ids.append(t)
        out = [self.tracks[t] for t in ids]
        while out and len(self.tracks[shard[j]].audio) + sum(len(t.audio) for t in out) > 64:
            out.pop()
        return out

    def __iter__(self):
        import random
        shard = self.shard()
        self.batcher.rng = random.Random((self.seed * 1000003 + self.epoch) * 4099 + self.rank)
        for i in range(0, len(shard), self.per):
            if self.n_partners:
                built = [self.batcher.build(self.tracks[shard[j]], partners=self.partners_of(shard, j))
                         for j in range(i, min(i + self.per, len(shard)))]
                yield tuple(torch.cat([b[k] for b in built]) for k in range(len(built[0])))
                continue
            built = [self.batcher.build(self.tracks[t]) for t in shard[i:i + self.per]]
            yield tuple(torch.cat([b[k] for b in built]) for k in range(len(built[0])))


def stem_loaders(cfg, opts, device, world=1, rank=0, with_prev=False):
    """(train StemLoader, validation StemLoader or None) over `+stem_root` / `+stem_val_root`; the row geometry is the
    config's (`mel_length`, `event_length`, `num_rows_per_batch`, `split_frame_length`, `dataloader.train.batch_size`
    tracks per step)."""
    from mrmt3 import stems
    from mrmt3.batching import StemMixBatcher
    geom = dict(mel_length=int(cfg.mel_length), event_length=int(cfg.event_length),
                num_rows_per_batch=int(cfg.num_rows_per_batch), split_frame_length=int(cfg.get("split_frame_length", 2000)))
    per = int(cfg.dataloader.train.batch_size)
    native = dict(any_rate=True) if opts.get("native_rate") else {}
    if opts.get("device_labels"):
        geom.update(device_labels=True, with_prev=with_prev)
    train = StemLoader(stems.load_stem_folder(opts["root"], **native),
                       StemMixBatcher(device, keep_prob=opts["keep"], min_stems=opts["min_stems"], gain_db=opts["gain_db"],
                                      pitch_shift=opts.get("pitch_shift", 0), cross_track=bool(opts.get("cross")),
                                      cross_prob=opts.get("cross_prob", 0.5), per_row_shift=bool(opts.get("shift_per_row")),
                                      **geom),
                       per, cfg.seed, rank, world, partners=opts.get("cross", 0))
    val = None
    if opts["val_root"] is not None:
        val = StemLoader(stems.load_stem_folder(opts["val_root"], **native), StemMixBatcher(device, is_deterministic=True, **geom),
                         1, cfg.seed, rank, world, shuffle=False)
    return train, val


def val_notes_options(cfg, stem):
    """None without `+val_notes=true`; else the number of validation tracks each rank transcribes (`+val_notes_tracks=K`,
    0: every track of its shard).  Needs `+stem_val_root`: the tracks' note tables are the reference."""
    raw = cfg.get("val_notes")
    if raw is None or str(raw).lower() not in _TRUTHY:
        if raw is not None and str(raw).lower() not in ("false", "0", "no", "off"):
            raise ValueError("val_notes must be true or false, got %r" % (raw,))
        return None
    if stem is None or stem.get("val_root") is None:
        raise ValueError("+val_notes=true scores transcriptions of the validation tracks: it needs +stem_root and "
                         "+stem_val_root")
    k = cfg.get("val_notes_tracks", 0)
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError("val_notes_tracks must be an int >= 0 (0: every track), got %r" % (k,))
    return int(k)


def full_mix(track, sample_rate=16000):
    """The deterministic full mix of a stem track as one recording: every stem at gain 1, from sample 0."""
    if track.rates is not None and any(int(r) != sample_rate for r in track.rates):
        raise ValueError("val_notes transcribes stems at the model's %d Hz; track %s has %r" % (sample_rate, track.name,
                                                                                                 track.rates))
    mix = np.zeros(track.n_samples, np.float32)
    for a in track.audio:
        mix[:len(a)] += a
    return mix


def val_frames_option(cfg, val_notes) -> bool:
    """`+val_frames=true`: the frame F1 beside the note-level numbers; it needs `+val_notes=true`."""
    raw = cfg.get("val_frames")
    if raw is None or str(raw).lower() in ("false", "0", "no", "off"):
        return False
    if str(raw).lower() not in _TRUTHY:
        raise ValueError("val_frames must be true or false, got %r" % (raw,))
    if val_notes is None:
        raise ValueError("+val_frames=true scores the frames of the notes +val_notes=true transcribes: it needs +val_notes=true")
    return True


def validate_notes(model, tracks, device, estimates=None, max_length=1024, frames=False) -> dict:
    """Note-level validation: the full mix of every track is transcribed by the model's inference path with the
    notes decoded on the device (`InferenceHandler.inference_many(return_tables=True)`), and scored there against the
    track's note table (`mrmt3.scoring.score_tables`, one launch for all tracks).  The NOTES THEMSELVES are scored, not a
    MIDI round trip: no file is written and read back, so no time is quantised to MIDI ticks on the way.  The weights are
    the model's as they stand (the training weights).
    `estimates`: a `mrmt3.notes.DeviceNotes` with one recording per track to score instead of transcribing.
    Returns {"tracks": n scored, "onset_f1": the SUM over the tracks of the instrument-agnostic onset F1,
    "onset_program_f1": the sum of "Onset + program F1 (flat)", "per_track": the tracks' score dicts}: sums and a count,
    so that ranks can be added like `val_loss`.  A track the host scorer would refuse (a reference note that does not
    end after it starts) is left out of the sums and carries its ValueError in `per_track`.
    `frames`: one launch of the frame kernel more, and "frame_f1", the sum of the tracks' "Frame F1"."""
    from mrmt3 import labels, scoring
    from mrmt3.notes import DeviceNotes
    tracks = list(tracks)
    out = {"tracks": 0, "onset_f1": 0.0, "onset_program_f1": 0.0, "per_track": []}
    if frames:
        out["frame_f1"] = 0.0
    if not tracks:
        return out
    if estimates is None:
        import inference
        was_training = model.training
        model.eval()
        try:
            handler = inference.InferenceHandler(model=model, device=device)
            estimates = handler.inference_many([full_mix(t) for t in tracks], max_length=max_length, return_tables=True)
        finally:
            model.train(was_training)
    refs = []
    for t in tracks:
        table = labels.note_table(t)
        refs.append(DeviceNotes.from_note_table(torch.from_numpy(table.times).to(device), torch.from_numpy(table.meta).to(device)))
    out["per_track"] = scoring.score_tables(DeviceNotes.concat(refs), estimates, families=("on", "flat"), errors="return",
                                            frames=frames)
    for got in out["per_track"]:
        if isinstance(got, Exception):
            continue
        out["tracks"] += 1
        out["onset_f1"] += got["Onset F1"]
        out["onset_program_f1"] += got["Onset + program F1 (flat)"]
        if frames:
            out["frame_f1"] += got["Frame F1"]
    return out


def accumulate_grad_batches(cfg) -> int:
    """Micro-batches per optimizer step: `trainer.accumulate_grad_batches`, else a top-level `grad_accum`, else 1."""
    tr = cfg.get("trainer")
    n = tr.get("accumulate_grad_batches") if tr is not None else None
    if n is None:
        n = cfg.get("grad_accum")
    return 1 if n is None else int(n)


_TRUTHY = ("1", "true", "yes", "on")


def gradient_clipping(cfg):
    """(gradient_clip_val or None, algorithm) from `trainer.gradient_clip_val` / `trainer.gradient_clip_algorithm`, as
    Lightning reads them: no value, null or 0 means no clipping; the algorithm defaults to "norm"."""
    from mrmt3.trainer import clip_options
    tr = cfg.get("trainer")
    val = tr.get("gradient_clip_val") if tr is not None else None
    algo = tr.get("gradient_clip_algorithm") if tr is not None else None
    algo = "norm" if algo is None else str(algo)
    val = None if val is None or str(val).lower() in ("", "none", "null") else float(val)
    val = None if val == 0 else val
    clip_options(val, algo)                      # the trainer's own validation: an unknown algorithm is a ValueError naming it
    return val, algo


def loss_options(cfg):
    """(label_smoothing, z_loss) from the top-level keys of those names (absent or null: 0), validated like the trainer's
    arguments: 0 <= label_smoothing < 1, z_loss >= 0, else a ValueError naming the key."""
    from mrmt3.lib import ce_options
    vals = []
    for key in ("label_smoothing", "z_loss"):
        raw = cfg.get(key)
        if raw is None or str(raw).lower() in ("", "none", "null"):
            vals.append(0.0)
            continue
        try:
            vals.append(float(raw))
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, got %r" % (key, raw)) from None
    _, eps, z = ce_options(*vals)
    return eps, z


def _pattern_list(cfg, key):
    """A top-level list of fnmatch patterns (absent or null: None).  Anything but a list of strings is a ValueError
    naming the key; whether a pattern matches a parameter is the trainer's check."""
    raw = cfg.get(key)
    if raw is None or (isinstance(raw, str) and raw.lower() in ("", "none", "null")):
        return None
    if isinstance(raw, str) or not hasattr(raw, "__iter__"):
        raise ValueError("%s must be a list of patterns, e.g. +%s='[\"encoder.*\"]', got %r" % (key, key, raw))
    out = list(raw)
    for pat in out:
        if not isinstance(pat, str) or not pat:
            raise ValueError("%s must be a list of non-empty strings, got the entry %r" % (key, pat))
    return out or None


EXPORT_CHOICES = ("train", "ema")


def group_options(cfg):
    """(frozen, no_decay, ema_decay, export) from the top-level keys `freeze`, `no_decay`, `ema_decay` and
    `export_weights`, validated like the loss options: a ValueError names the key."""
    from mrmt3.params import ema_decay_option
    frozen, no_decay = _pattern_list(cfg, "freeze"), _pattern_list(cfg, "no_decay")
    raw = cfg.get("ema_decay")
    if raw is None or str(raw).lower() in ("", "none", "null"):
        ema = None
    else:
        try:
            ema = float(raw)
        except (TypeError, ValueError):
            raise ValueError("ema_decay must be a number in (0, 1), got %r" % (raw,)) from None
        if isinstance(raw, bool):
            raise ValueError("ema_decay must be a number in (0, 1), got %r" % (raw,))
        ema = ema_decay_option(ema)
    export = str(cfg.get("export_weights", "train")).lower()
    if export not in EXPORT_CHOICES:
        raise ValueError("export_weights must be one of %s, got %r" % (EXPORT_CHOICES, export))
    if export == "ema" and ema is None:
        raise ValueError("export_weights=ema needs ema_decay")
    return frozen, no_decay, ema, export


def format_step_line(it, loss, nll=None, grad_norm=None):
    """Rank 0's log line of optimizer step `it`: `step N train_loss X`, then `nll Y` when a loss option is on and
    `grad_norm G` when the clipping tail is (floats; None leaves the field out)."""
    line = f"step {it} train_loss {loss:.4f}"
    if nll is not None:
        line += f" nll {nll:.4f}"
    if grad_norm is not None:
        line += f" grad_norm {grad_norm:.4f}"
    return line


def resume_position(global_step, steps_per_epoch, accumulate=1):
    """(epoch, batches of that epoch already consumed) for a run that has taken `global_step` optimizer steps.  The
    position is derived from the step count alone: a checkpoint's `epoch` field is the epoch in progress OR the one
    just completed depending on when it was written, the step count is unambiguous.  `steps_per_epoch` is
    the loader's length in batches; with `accumulate` = N batches per optimizer step an epoch takes ceil(len / N) steps
    (the last one possibly partial), so the batches consumed are N per step taken in the epoch."""
    if steps_per_epoch <= 0:
        return 0, 0
    per_epoch = -(-steps_per_epoch // accumulate)
    return global_step // per_epoch, (global_step % per_epoch) * accumulate


def loader_batches(loader, device, epochs, max_steps, start_epoch=0, start_step=0, sampler=None, skip=0, accumulate=1):
    """(epoch, inputs, targets, targets_prev) from the reference's collated batches, moved to the device.  A resumed
    run continues at (start_epoch, start_step) and drops the first `skip` batches of that epoch (the ones the
    interrupted run consumed): `max_steps` counts global optimizer steps, like Lightning's — with `accumulate` = N an
    optimizer step ends at every N-th batch of an epoch and at its last batch."""
    n = start_step
    try:
        per_epoch = len(loader)
    except TypeError:
        per_epoch = None
    bs = getattr(loader, "batch_sampler", None)
    index_skip = isinstance(bs, SkippingBatchSampler)
    for ep in range(start_epoch, epochs):
        if index_skip:
            bs.set_epoch(ep)                 # a different shuffle per epoch: a function of (seed, epoch), on every rank
            bs.skip = skip if ep == start_epoch else 0
        elif sampler is not None:
            sampler.set_epoch(ep)
        for bi, batch in enumerate(loader):
            if not index_skip and ep == start_epoch and bi < skip:
                continue                     # (a loader of another kind: the consumed batches are loaded and dropped)
            if max_steps is not None and n >= max_steps:
                return
            inputs, targets = batch[0], batch[1]
            prev = batch[2] if len(batch) > 2 else None
            yield ep, inputs.to(device, non_blocking=True), targets.to(device, non_blocking=True), \
                (None if prev is None else prev.to(device, non_blocking=True))
            pos = bi + (skip if index_skip and ep == start_epoch else 0)      # the batch's index in its epoch
            if accumulate == 1 or (pos + 1) % accumulate == 0 or (per_epoch is not None and pos + 1 == per_epoch):
                n += 1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config-dir", "--config-path", dest="config_dir", required=True)   # both spellings appear in the reference's scripts
    ap.add_argument("--config-name", default="config")
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args(argv)
    cfg = hydra_lite.compose(a.config_dir, a.config_name, a.overrides)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.manual_seed(int(cfg.seed))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=device)
    task = hydra_lite.instantiate(cfg.model, optim_cfg=cfg.optim, eval_cfg=cfg.get("eval"))
    assert cfg.model_type == cfg.model._target_.split(".")[-1], "model_type and model target mismatched"   # train.py:36
    task.to(device)
    from mrmt3.trainer import Trainer
    from utils import cosine_warmup_lambda
    finetune = type(task).__name__.endswith("FineTune")
    lam = None if finetune else cosine_warmup_lambda(int(cfg.optim.warmup_steps),
                                                     int(cfg.optim.num_steps_per_epoch) * int(cfg.optim.num_epochs),
                                                     min_lr=float(cfg.optim.min_lr))
    # packed decoder rows (mrmt3/packing.py): `+pack_targets=true`; absent, MRMT3_PACK_TARGETS decides (default off)
    pack = cfg.get("pack_targets")
    pack = None if pack is None else str(pack).lower() in _TRUTHY
    accum = accumulate_grad_batches(cfg)
    clip_val, clip_algo = gradient_clipping(cfg)
    skip_nonfinite = str(cfg.get("skip_nonfinite", False)).lower() in _TRUTHY
    label_smoothing, z_loss = loss_options(cfg)
    frozen, no_decay, ema_decay, export = group_options(cfg)
    trainer = Trainer(task.model, lr=float(cfg.optim.lr), lr_lambda=lam,
                      weighted_loss=type(task).__name__ == "MT3NetWeightedLoss", pack_targets=pack,
                      accumulate_grad_batches=accum, gradient_clip_val=clip_val, gradient_clip_algorithm=clip_algo,
                      skip_nonfinite=skip_nonfinite, label_smoothing=label_smoothing, z_loss=z_loss, frozen=frozen,
                      no_decay=no_decay, ema_decay=ema_decay)

    def step_line(it, loss):
        """Rank 0's log line of optimizer step `it` (reads the device: only at the logging cadence)."""
        return format_step_line(it, loss.item(), trainer.last_nll.item() if trainer.loss_reg else None,
                                trainer.last_grad_norm.item() if trainer.clip_on else None)

    task.model.engine.seed = int(cfg.seed)
    with_prev = "WithPrev" in type(task).__name__
    synthetic = bool(cfg.get("synthetic", False))
    max_steps = cfg.get("max_steps")
    max_steps = None if max_steps is None else int(max_steps)
    train_loader = val_loader = sampler = None
    stem = None if synthetic else stem_options(cfg, with_prev)
    val_notes = val_notes_options(cfg, stem)
    val_frames = val_frames_option(cfg, val_notes)
    if stem is not None:
        train_loader, val_loader = stem_loaders(cfg, stem, device, world, rank, with_prev)
        sampler = train_loader                   # (`set_epoch`: the track order is a function of (seed, epoch))
    elif not synthetic:
        train_loader, val_loader, sampler = real_loaders(cfg, world, rank)
    start, start_epoch, skip, resumed = 0, 0, 0, False
    path = cfg.get("path")
    if path is not None and str(path) != "":
        path = str(path)
        if path.endswith(".ckpt"):
            start = trainer.resume(path)
            if train_loader is not None:
                start_epoch, skip = resume_position(start, len(train_loader), accum)
            if rank == 0:
                print(f"Resuming from {path} at step {start}, epoch {start_epoch} (+{skip} batches)", flush=True)
        elif path.endswith(".pth"):
            if rank == 0:
                print(f"Loading weights from {path}...", flush=True)
            trainer.resume(path)
        else:
            raise ValueError(f"Invalid extension for path: {path}")
        resumed = True
    # every rank draws its own dropout masks (torch DDP: one generator per process), not world copies of one mask
    # (after the resume, which restores the seed rank 0 saved)
    task.model.engine.seed += 1000003 * rank
    log_every = max(1, int(cfg.trainer.get("log_every_n_steps", 100)))
    if synthetic:
        steps = 10 if max_steps is None else max_steps
        for k, (audio, labels, prev) in enumerate(synthetic_batches(cfg, rank, device, steps * accum, with_prev)):
            loss = trainer.train_step(audio, labels, prev, audio=True)
            if trainer.pending_micro_batches:
                continue                 # (mid-cycle: no optimizer step yet)
            it = start + (k + 1) // accum - 1
            if rank == 0 and (it % log_every == 0 or it == start + steps - 1):
                print(step_line(it, loss), flush=True)
    else:
        val_every = max(1, int(cfg.trainer.get("check_val_every_n_epoch", 1)))
        it, last_ep, loss = start, start_epoch, None

        def validate(ep):
            """val_loss = mean over the batches of ALL ranks (each rank holds a shard of the validation set)."""
            if val_loader is None:               # (+stem_root without +stem_val_root)
                return
            acc = torch.zeros(2, device=device, dtype=torch.float64)
            for b in val_loader:
                prev = b[2].to(device) if len(b) > 2 else None
                acc[0] += trainer.eval_loss(b[0].to(device), b[1].to(device), prev).double().sum()
                acc[1] += 1
            if world > 1:
                dist.all_reduce(acc, op=dist.ReduceOp.SUM)
            if rank == 0 and acc[1].item() > 0:
                print(f"epoch {ep} val_loss {(acc[0] / acc[1]).item():.4f}", flush=True)
            if val_notes is not None:            # (+val_notes=true: the training weights, the first tracks of the shard)
                shard = val_loader.shard()
                got = validate_notes(task.model, [val_loader.tracks[t] for t in shard[:val_notes or len(shard)]], device,
                                     max_length=int(cfg.get("event_length", 1024)), frames=val_frames)
                notes_acc = torch.tensor([got["onset_f1"], got["onset_program_f1"], got["tracks"], got.get("frame_f1", 0.0)],
                                         device=device, dtype=torch.float64)
                if world > 1:
                    dist.all_reduce(notes_acc, op=dist.ReduceOp.SUM)
                if rank == 0 and notes_acc[2].item() > 0:
                    f1, pf1 = (notes_acc[:2] / notes_acc[2]).tolist()
                    print(f"epoch {ep} val_onset_f1 {f1:.4f} val_onset_program_f1 {pf1:.4f}", flush=True)
                    if val_frames:
                        print(f"epoch {ep} val_frame_f1 {(notes_acc[3] / notes_acc[2]).item():.4f}", flush=True)
            if ema_decay is None:
                return
            acc.zero_()
            with trainer.ema_weights():
                for b in val_loader:
                    prev = b[2].to(device) if len(b) > 2 else None
                    acc[0] += trainer.eval_loss(b[0].to(device), b[1].to(device), prev).double().sum()
                    acc[1] += 1
            if world > 1:
                dist.all_reduce(acc, op=dist.ReduceOp.SUM)
            if rank == 0 and acc[1].item() > 0:
                print(f"epoch {ep} val_loss_ema {(acc[0] / acc[1]).item():.4f}", flush=True)

        def stepped(loss):
            """An optimizer step has run; `loss` is its last micro-batch's."""
            nonlocal it
            if rank == 0 and it % log_every == 0:
                print(step_line(it, loss), flush=True)
            it += 1

        if resumed:
            validate(start_epoch)        # the reference validates the loaded weights before fit (train.py:61-87)
        for ep, mel, labels, prev in loader_batches(train_loader, device, int(cfg.num_epochs), max_steps,
                                                    start_epoch, start, sampler, skip, accum):
            if ep != last_ep:
                if trainer.finish_accumulation():      # the epoch's partial accumulation cycle steps before validation
                    stepped(loss)
                if (last_ep + 1) % val_every == 0:
                    validate(last_ep)
            last_ep = ep
            loss = trainer.train_step(mel, labels, prev, audio=False)
            if not trainer.pending_micro_batches:
                stepped(loss)
        if trainer.finish_accumulation():
            stepped(loss)
        if rank == 0 and loss is not None and (it - 1) % log_every != 0:
            print(step_line(it - 1, loss), flush=True)
        if (last_ep + 1) % val_every == 0:
            validate(last_ep)
    if rank == 0 and trainer.clip_on:
        skipped = trainer.skipped_steps          # (every rank skips the same steps: the norm is of the exchanged gradient)
        if skipped > 0:
            print(f"skipped_steps {skipped}", flush=True)
    if rank == 0 and stem is not None and (stem.get("pitch_shift") or stem.get("native_rate")):
        from mrmt3 import lib
        print(f"resample_launches {lib.resample_launches()}", flush=True)      # (this rank's: shifted rows + uploaded stems)
    if rank == 0 and stem is not None and stem.get("device_labels"):
        from mrmt3 import lib
        print(f"label_launches {lib.label_launches()}", flush=True)            # (this rank's: one per track visit)
    if rank == 0:
        out_dir = os.path.join(str(cfg.get("output_dir", ".")), f"{cfg.model_type}_{cfg.dataset_type}",
                               "version_0", "checkpoints")
        os.makedirs(out_dir, exist_ok=True)
        trainer.save_checkpoint(os.path.join(out_dir, "last.ckpt"), epoch=0 if synthetic else last_ep)
        if ema_decay is not None:
            torch.save(trainer.ema_state_dict(), os.path.join(out_dir, "last_ema.pt"))
        if export == "ema":
            torch.save(trainer.ema_state_dict(), os.path.join(out_dir, "last.pt"))
        else:
            trainer.save_checkpoint(os.path.join(out_dir, "last.pt"))
        print(f"Saved model in {os.path.join(out_dir, 'last.pt')}.", flush=True)
    trainer.close()                      # captured graphs, then the library's own RCCL communicator (MRMT3_DDP_NATIVE), before torch's
    if world > 1:
        dist.destroy_process_group()
    return task


if __name__ == "__main__":
    main()
