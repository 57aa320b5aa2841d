"""GPU-resident batch construction from raw audio.

The reference builds every training row on a DataLoader worker CPU: split the song into chunks,
pick a run of chunks, pick a random mel_length window in each, compute that window's log-mel with
torchaudio, normalise, zero-pad, and ship 512 KB of mel per row (dataset/dataset_2_random.py:308-344,
281-306, 385-420).  Here the worker ships the recording ONCE (128 KB per 256 frames) and only the
crop DECISIONS are made on the host, with the same `random.randint` draws in the same order; the crops
are never materialised — `mrmt3_logmel_crops_fwd` reads each one straight out of the recording in
HBM and writes the padded `[B, mel_length, 512]` batch in one launch.

Target tokenisation (`_extract_target_sequence_with_indices`, `_run_length_encode_shifts`) stays on the
host and is passed in per row; `pad_targets` is the `_pad_length` target half.
"""
from __future__ import annotations

import random as _random
from dataclasses import dataclass

import numpy as np
import torch


@dataclass
class CropPlan:
    """One row per batch element, in frames (1 frame = hop_width samples) of the recording."""
    start_frame: np.ndarray      # int64 [B]
    valid_frames: np.ndarray     # int32 [B]  (< mel_length only for recordings shorter than one window)
    chunk_start: np.ndarray      # int64 [B]  start of the `_split_frame` chunk the crop was drawn from


def plan_crops(n_frames: int, mel_length: int = 256, num_rows_per_batch: int = 12, split_frame_length: int = 2000,
               is_deterministic: bool = False, rng=None) -> CropPlan:
    """Index arithmetic of `_split_frame` + row selection + `_random_chunk` for a recording of n_frames.
    `rng` is anything with `randint(a, b)` inclusive (default: the `random` module, like the reference), and
    is consumed in the reference's order: one draw for the run of chunks, then one per row."""
    rng = rng or _random
    chunks = [(s, split_frame_length) for s in range(0, n_frames, split_frame_length)
              if not s + split_frame_length >= n_frames]                    # last chunk dropped (:315-316)
    if not chunks:
        chunks = [(0, n_frames)]                                            # short song: the whole row (:325-326)
    if len(chunks) > num_rows_per_batch:
        first = 0 if is_deterministic else rng.randint(0, len(chunks) - num_rows_per_batch)
        chunks = chunks[first:first + num_rows_per_batch]
    starts, valid, cstart = [], [], []
    for s, n in chunks:
        slack = n - mel_length
        off = 0
        if slack >= 1 and not is_deterministic:                             # :332-338
            off = rng.randint(0, slack)
        starts.append(s + off)
        valid.append(min(mel_length, n))                                    # `_pad_length` zero-pads the rest
        cstart.append(s)
    return CropPlan(np.asarray(starts, np.int64), np.asarray(valid, np.int32), np.asarray(cstart, np.int64))


def pad_targets(targets, event_length: int = 1024, num_special_tokens: int = 3) -> torch.Tensor:
    """`_pad_length` target half (:294-305): truncate, +3, EOS, -100 padding; a target that already fills
    event_length gets neither EOS nor padding.  `targets`: list of 1-D int arrays -> int64 [B, event_length]."""
    out = np.full((len(targets), event_length), -100, np.int64)
    for i, t in enumerate(targets):
        t = np.asarray(t[:event_length], np.int64) + num_special_tokens
        out[i, :len(t)] = t
        if len(t) < event_length:
            out[i, len(t)] = 1
    return torch.from_numpy(out)


class DeviceBatcher:
    """recording on the GPU + crop plan -> `(inputs [B, mel_length, 512], targets [B, event_length])`, the
    pair `__getitem__` returns (:420), with `inputs` produced by one kernel launch."""

    def __init__(self, device, mel_length: int = 256, event_length: int = 1024, num_rows_per_batch: int = 12,
                 split_frame_length: int = 2000, is_deterministic: bool = False, spectrogram_config=None,
                 out_bf16: bool = False, rng=None):
        from contrib import spectrograms
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceBatcher builds batches on the GPU (no CPU fallback)")
        self.cfg = spectrogram_config or spectrograms.SpectrogramConfig()
        self.mel_length, self.event_length = mel_length, event_length
        self.num_rows, self.split_len = num_rows_per_batch, split_frame_length
        self.is_deterministic, self.out_bf16, self.rng = is_deterministic, out_bf16, rng
        self._sp = spectrograms

    def upload(self, samples) -> torch.Tensor:
        """host recording (numpy / tensor, any float dtype) -> f32 device tensor, padded to whole frames like
        `split_audio` (contrib/spectrograms.py:79-90).  Pinned staging + async copy."""
        x = torch.as_tensor(np.asarray(samples), dtype=torch.float32).reshape(-1)
        hop = self.cfg.hop_width
        pad = (-x.numel()) % hop
        if pad:
            x = torch.cat([x, x.new_zeros(pad)])
        return x.pin_memory().to(self.device, non_blocking=True)

    def plan(self, n_frames: int) -> CropPlan:
        return plan_crops(n_frames, self.mel_length, self.num_rows, self.split_len, self.is_deterministic, self.rng)

    def mel(self, audio_dev: torch.Tensor, plan: CropPlan) -> torch.Tensor:
        starts = torch.from_numpy(plan.start_frame)
        vf = torch.from_numpy(plan.valid_frames)
        return self._sp.logmel_crops(audio_dev, starts, self.mel_length, self.cfg, normalize=True,
                                     valid_frames=vf, out_bf16=self.out_bf16)

    def build(self, audio_dev: torch.Tensor, targets_for_crop, plan: CropPlan | None = None):
        """`targets_for_crop(start_frame, n_frames) -> 1-D int array` is the host tokeniser for one crop."""
        plan = plan or self.plan(audio_dev.numel() // self.cfg.hop_width)
        mel = self.mel(audio_dev, plan)
        tg = pad_targets([targets_for_crop(int(s), int(v)) for s, v in zip(plan.start_frame, plan.valid_frames)],
                         self.event_length)
        return mel, tg.to(self.device, non_blocking=True)


# ---- stem-mix rows -------------------------------------------------------------------------------------------

@dataclass
class StemMixPlan:
    """`CropPlan` of the track plus, per row, which stems sound and how loud."""
    crops: CropPlan
    keep: np.ndarray             # bool [B, S]
    gain: np.ndarray             # float32 [B, S], 0 where a stem is not kept
    shift: int = 0               # pitch shift of the whole plan in semitones; 0: the track as it is
    step: int = 1 << 32          # 32.32 input samples per output sample, ratio_step(2 ** (shift / 12))


def plan_stem_mix(n_frames: int, n_stems: int, mel_length: int = 256, num_rows_per_batch: int = 12,
                  split_frame_length: int = 2000, keep_prob: float = 0.75, min_stems: int = 1, gain_db: float = 6.0,
                  is_deterministic: bool = False, rng=None) -> StemMixPlan:
    """Row plan of one track.  `rng` is anything with `randint(a, b)` inclusive, `random()` and `uniform(a, b)` (default:
    the `random` module) and is consumed in this order:
      1. the crop draws of `plan_crops`, unchanged: one for the run of chunks, then one per row;
      2. then row by row: one `random()` per stem in stem order (kept iff < keep_prob); while fewer than
         min(min_stems, n_stems) are kept, one `randint(0, len(dropped) - 1)` picking a dropped stem (in stem order) to
         keep; then one `uniform(-gain_db, gain_db)` per KEPT stem in stem order, the gain being 10^(dB / 20) in f32.
    `is_deterministic`: every stem at gain 1 and no draw at all (the validation form)."""
    rng = rng or _random
    crops = plan_crops(n_frames, mel_length, num_rows_per_batch, split_frame_length, is_deterministic, rng)
    B = len(crops.start_frame)
    keep = np.ones((B, n_stems), bool)
    gain = np.ones((B, n_stems), np.float32)
    if is_deterministic:
        return StemMixPlan(crops, keep, gain)
    need = min(int(min_stems), n_stems)
    for b in range(B):
        keep[b] = [rng.random() < keep_prob for _ in range(n_stems)]
        while keep[b].sum() < need:
            dropped = np.nonzero(~keep[b])[0]
            keep[b, dropped[rng.randint(0, len(dropped) - 1)]] = True
        for s in range(n_stems):
            gain[b, s] = np.float32(10.0 ** (rng.uniform(-gain_db, gain_db) / 20.0)) if keep[b, s] else np.float32(0)
    return StemMixPlan(crops, keep, gain)


def stem_pool_layout(lengths, hop: int):
    """Stems end to end in one pool, each starting on a whole hop: (offsets int64 [S], pool_samples)."""
    padded = [-(-int(n) // hop) * hop for n in lengths]
    offsets = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    return offsets, int(sum(padded))


def mix_tables(plan: StemMixPlan, offsets, lengths, hop: int):
    """The kernel's tables for a plan over a pool laid out by `stem_pool_layout`: (start_frames int64 [B, S] in hops of
    the pool, src_end int64 [B, S] in samples, src_gain float32 [B, S]).  A crop that starts at or behind the end of a
    (shorter) stem has nothing of that stem to read: the source's table gain is 0, which the kernel does not read at all
    (its start is left at the stem's last hop).  The plan's own `gain` and `keep` — the labels — are untouched."""
    offsets, lengths = np.asarray(offsets, np.int64), np.asarray(lengths, np.int64)
    end = np.broadcast_to(offsets + lengths, plan.gain.shape).copy()
    start = offsets[None, :] // hop + plan.crops.start_frame[:, None]
    over = start * hop >= end
    start = np.where(over, end // hop, start)
    gain = np.where(over, np.float32(0), plan.gain).astype(np.float32)
    return start.astype(np.int64), end, np.ascontiguousarray(gain)


def resample_tables(plan: StemMixPlan, offsets, lengths, hop: int):
    """The resampler's tables for a pitch-shifted plan over a pool laid out by `stem_pool_layout`:
    (src_pos, src_begin, src_end, src_step int64 [B, S], src_gain float32 [B, S], src_filt int32 [B, S] all 0,
    valid_samples int64 [B]).  Source s of row b starts at (offset_s << 32) + start_frame_b * hop * step and is bounded by
    its own stem.  The stretched stem has `out_length(len_s, step)` samples; a crop that starts at or behind them has
    nothing of that stem to read and gets table gain 0 as in `mix_tables` (its position is left at the stem's start) —
    which covers every source whose first tap lies at or behind its stem's end."""
    from mrmt3.resample import out_length
    offsets, lengths = np.asarray(offsets, np.int64), np.asarray(lengths, np.int64)
    shape = plan.gain.shape
    step = int(plan.step)
    begin = np.broadcast_to(offsets, shape).copy()
    end = np.broadcast_to(offsets + lengths, shape).copy()
    start = plan.crops.start_frame.astype(np.int64)[:, None] * hop                      # in stretched samples
    over = start >= np.array([out_length(int(n), step) for n in lengths], np.int64)[None, :]
    pos = np.where(over, begin << 32, (begin << 32) + start * step)
    gain = np.where(over, np.float32(0), plan.gain).astype(np.float32)
    return (pos.astype(np.int64), begin, end, np.full(shape, step, np.int64), np.ascontiguousarray(gain),
            np.zeros(shape, np.int32), plan.crops.valid_frames.astype(np.int64) * hop)


def check_mix_tables(start_frames, src_end, src_gain, pool_samples: int, hop: int):
    """Host check of the tables before they are uploaded: every gain finite; for every source that sounds (gain != 0)
    0 <= start <= end <= pool_samples.  A ValueError names the row.  (The kernel is safe without it — it clamps — but a
    table that needs clamping is a planning bug, and the host is where it can be reported.)"""
    start = np.asarray(start_frames, np.int64) * hop
    end, gain = np.asarray(src_end, np.int64), np.asarray(src_gain, np.float32)
    if not (start.shape == end.shape == gain.shape and gain.ndim == 2):
        raise ValueError("stem mix tables: start, end and gain must share one [rows, sources] shape, got %s %s %s"
                         % (start.shape, end.shape, gain.shape))
    if not 1 <= gain.shape[1] <= 64:
        raise ValueError("stem mix tables: %d sources per row, the kernel takes 1 to 64" % gain.shape[1])
    for b in range(gain.shape[0]):
        if not np.isfinite(gain[b]).all():
            raise ValueError("stem mix tables: row %d has a gain that is not finite: %s" % (b, gain[b].tolist()))
        on = gain[b] != 0
        if (start[b][on] < 0).any() or (end[b][on] > pool_samples).any():
            raise ValueError("stem mix tables: row %d points outside the pool of %d samples (start %s, end %s)"
                             % (b, pool_samples, start[b][on].tolist(), end[b][on].tolist()))
        if (start[b][on] > end[b][on]).any():
            raise ValueError("stem mix tables: row %d starts behind its stem's end (start %s, end %s)"
                             % (b, start[b][on].tolist(), end[b][on].tolist()))


class StemMixBatcher:
    """A track's stems on the GPU + a row plan -> `(mel [B, mel_length, 512], targets [B, event_length])`: every row a
    random sub-mix of the stems at random gains, mixed inside the log-mel kernel's load (`mrmt3_logmel_mix_fwd`, one
    launch, nothing materialised), labelled with the notes of exactly the stems that sound.

    The targets of a row are BY DEFINITION `Tokenizer.row_targets` of the tokenisation of
    `mrmt3.stems.merged_note_sequence(track, kept)` at the track's length; tokenisations are cached per (track, subset)
    (tests hold the cached path to the definition).  `plan` / `row_targets` are host code and run without a GPU; `build`
    needs one (no CPU fallback).  Stems are uploaded once per track through pinned staging and kept in a device cache of
    at most `cache_bytes` (least recently used track dropped first; the track in use always stays).

    `pitch_shift=S` > 0: every plan first draws one shift of k semitones in [-S, S], clamped so that no label
    leaves the codec's pitches; the whole track visit is played at 2^(k/12) times its speed — the rows are resampled and
    mixed by `mrmt3_resample_mix_fwd` and go through `mrmt3_logmel_fwd`, the labels are those of
    `mrmt3.stems.speed_note_sequence`.  k = 0 and `pitch_shift=0` are the launch above, untouched.  A stem whose
    `track.rates` entry is not the config's rate is resampled on the device, once, when the track is uploaded.

    `device_labels=True`: `build` makes the targets with one launch of `mrmt3_label_rows_fwd` over the track's
    note table, which lives on the device beside the pool; no tokenisation of the whole track, and the same targets.  It
    accepts only the tokenizer configuration the kernel implements (ties, no onsets-only, training trim, no token-order
    augmentation, the codec's own velocity bins): a ValueError names the option.  `with_prev=True` (needs
    `device_labels`) adds `targets_prev`, `Tokenizer.row_targets_prev` row by row, for the `*WithPrev` models.  With both
    off every call and every bit is what it was.

    `cross_track=True` / `per_row_shift=True` (both need `device_labels`): `build(track, partners=...)` makes
    rows of VIRTUAL tracks planned by `plan_cross` — stems of up to 3 partner tracks borrowed into a row with probability
    `cross_prob` each, every part at its own start, and with `per_row_shift` its own transposition within `pitch_shift`.
    With `cross_track` the cache is an arena: one device allocation for the audio of every cached track (both audio
    kernels take ONE pool) and one pair for their note tables, `cache_bytes` in all; `pool(track)` is the track's slot.
    With both off nothing of this runs."""

    def __init__(self, device, mel_length: int = 256, event_length: int = 1024, num_rows_per_batch: int = 12,
                 split_frame_length: int = 2000, keep_prob: float = 0.75, min_stems: int = 1, gain_db: float = 6.0,
                 is_deterministic: bool = False, tokenizer=None, rng=None, cache_bytes: int = 8 << 30,
                 spectrogram_config=None, out_bf16: bool = False, pitch_shift: int = 0, device_labels: bool = False,
                 with_prev: bool = False, cross_track: bool = False, cross_prob: float = 0.5, per_row_shift: bool = False):
        from collections import OrderedDict
        from contrib import spectrograms
        from mrmt3.tokenizer import Tokenizer
        if isinstance(pitch_shift, bool) or not isinstance(pitch_shift, (int, np.integer)) or not 0 <= pitch_shift <= 24:
            raise ValueError("pitch_shift must be an int in [0, 24] (semitones), got %r" % (pitch_shift,))
        if not 0.0 <= keep_prob <= 1.0:
            raise ValueError("keep_prob must be in [0, 1], got %r" % (keep_prob,))
        if min_stems < 1:
            raise ValueError("min_stems must be at least 1, got %r" % (min_stems,))
        if not (gain_db >= 0 and np.isfinite(gain_db)):
            raise ValueError("gain_db must be finite and >= 0, got %r" % (gain_db,))
        self.device = torch.device(device)
        self.cfg = spectrogram_config or spectrograms.SpectrogramConfig()
        self.mel_length, self.event_length = mel_length, event_length
        self.num_rows, self.split_len = num_rows_per_batch, split_frame_length
        self.keep_prob, self.min_stems, self.gain_db = float(keep_prob), int(min_stems), float(gain_db)
        self.is_deterministic, self.out_bf16, self.rng = is_deterministic, out_bf16, rng
        self.pitch_shift = int(pitch_shift)
        self.tokenizer = tokenizer or Tokenizer(spectrogram_config=self.cfg)
        self.device_labels, self.with_prev = bool(device_labels), bool(with_prev)
        if self.with_prev and not self.device_labels:
            raise ValueError("with_prev=True needs device_labels=True: targets_prev is built by the label kernel only")
        if self.device_labels:
            from mrmt3.labels import label_codec
            self._codec = label_codec(self.tokenizer)        # ValueError: a tokenizer option the kernel does not implement
        self.cross_track, self.per_row_shift, self.cross_prob = bool(cross_track), bool(per_row_shift), float(cross_prob)
        for name, on in (("cross_track", self.cross_track), ("per_row_shift", self.per_row_shift)):
            if on and not self.device_labels:
                raise ValueError("%s=True needs device_labels=True: on the host path every such row would need a "
                                 "tokenisation of its own" % name)
        if not 0.0 <= self.cross_prob <= 1.0:
            raise ValueError("cross_prob must be in [0, 1], got %r" % (cross_prob,))
        if self.cross_track and self.pitch_shift > 0 and not self.per_row_shift:
            raise ValueError("cross_track=True with pitch_shift needs per_row_shift=True: every part has its own shift range")
        self._arena = None                   # cross_track: (TrackArena, audio, note times, note meta), made at the first upload
        self._in_use = ()                    # names of the tracks of the build in progress: never evicted
        self._filters = OrderedDict()        # tuple of steps -> stacked filter tables on the device
        self._notes = {}                     # track.name -> (NoteTable on the device), beside the track's pool
        self.host_label_rows = 0             # rows the label kernel handed back (status != 0), rebuilt on the host
        self.cache_bytes = int(cache_bytes)
        self._pools = OrderedDict()          # track.name -> (pool on the device, offsets, lengths), least recent first
        self._feats = OrderedDict()          # (track.name, kept, shift) -> Tokenizer.tokenize(...)
        self.uploads = 0                     # tracks copied to the device so far (a cache hit does not count)
        self._sp = spectrograms

    # ---- host ----------------------------------------------------------------------------------------------------
    def lengths(self, track, step: int = 1 << 32) -> list:
        """Samples of every stem at the config's rate, played at step / 2^32 times its speed."""
        from mrmt3.resample import out_length
        lengths = track.lengths(self.cfg.sample_rate)
        return lengths if step == 1 << 32 else [out_length(n, step) for n in lengths]

    def n_samples(self, track, step: int = 1 << 32) -> int:
        """The (stretched) track's length: its longest stem."""
        return max(self.lengths(track, step))

    def n_frames(self, track, step: int = 1 << 32) -> int:
        return -(-self.n_samples(track, step) // self.cfg.hop_width)

    def plan(self, track) -> StemMixPlan:
        """With `pitch_shift` S > 0 (and not deterministic) ONE `randint(-S, S)` comes first: the shift of the whole
        track visit, clamped into `mrmt3.stems.shift_range(track)`; every draw of `plan_stem_mix` follows unchanged, over
        the frames of the stretched track."""
        shift, step = 0, 1 << 32
        if self.pitch_shift > 0 and not self.is_deterministic:
            from mrmt3.resample import ratio_step
            from mrmt3.stems import shift_range
            lo, hi = shift_range(track)
            shift = max(lo, min(hi, int((self.rng or _random).randint(-self.pitch_shift, self.pitch_shift))))
            step = ratio_step(2.0 ** (shift / 12.0))
        plan = plan_stem_mix(self.n_frames(track, step), len(track.audio), self.mel_length, self.num_rows, self.split_len,
                             self.keep_prob, self.min_stems, self.gain_db, self.is_deterministic, self.rng)
        plan.shift, plan.step = shift, step
        return plan

    def _tokenized(self, track, kept, shift: int = 0, step: int = 1 << 32):
        from mrmt3.stems import merged_note_sequence, speed_note_sequence
        key = (track.name, kept, int(shift))
        if key in self._feats:
            self._feats.move_to_end(key)
            return self._feats[key]
        ns = merged_note_sequence(track, kept)
        if shift != 0:
            ns = speed_note_sequence(ns, shift, step)
        feats = self.tokenizer.tokenize(ns, self.n_samples(track, step))
        self._feats[key] = feats
        while len(self._feats) > 64:
            self._feats.popitem(last=False)
        return feats

    def _host_row(self, track, plan: StemMixPlan, b: int, prev: bool = False):
        """Token ids of row b of the plan, or of its previous window, by the host tokenizer."""
        kept = tuple(int(s) for s in np.nonzero(plan.keep[b])[0])
        feats = self._tokenized(track, kept, plan.shift, plan.step)
        if prev:
            return self.tokenizer.row_targets_prev(feats, int(plan.crops.start_frame[b]), int(plan.crops.chunk_start[b]),
                                                   self.mel_length)
        return self.tokenizer.row_targets(feats, int(plan.crops.start_frame[b]), int(plan.crops.valid_frames[b]))

    def row_targets(self, track, plan: StemMixPlan):
        """Token ids of every row of the plan (a list of 1-D int arrays, before `pad_targets`)."""
        return [self._host_row(track, plan, b) for b in range(len(plan.crops.start_frame))]

    def tables(self, track, plan: StemMixPlan):
        """(start_frames, src_end, src_gain, pool_samples) of the plan on the host, checked."""
        hop = self.cfg.hop_width
        lengths = self.lengths(track)
        offsets, total = stem_pool_layout(lengths, hop)
        start, end, gain = mix_tables(plan, offsets, lengths, hop)
        check_mix_tables(start, end, gain, total, hop)
        return start, end, gain, total

    def shifted_tables(self, track, plan: StemMixPlan):
        """(src_pos, src_begin, src_end, src_step, src_gain, src_filt, valid_samples, pool_samples) of a pitch-shifted plan
        on the host, checked: the resampler's tables over the same pool (one filter table, index 0)."""
        from mrmt3.resample import check_resample_tables
        hop = self.cfg.hop_width
        lengths = self.lengths(track)
        offsets, total = stem_pool_layout(lengths, hop)
        tabs = resample_tables(plan, offsets, lengths, hop)
        check_resample_tables(*tabs[:6], total, 1)
        return tabs + (total,)

    # ---- device --------------------------------------------------------------------------------------------------
    def pool(self, track) -> torch.Tensor:
        """The track's stems end to end on the device (each padded to whole hops), uploaded once and cached."""
        if self.device.type != "cuda":
            raise RuntimeError("StemMixBatcher builds batches on the GPU (no CPU fallback)")
        if track.name in self._pools:
            self._pools.move_to_end(track.name)
            if self._arena is not None:
                self._arena[0].touch(track.name)
            return self._pools[track.name]
        hop = self.cfg.hop_width
        rate = self.cfg.sample_rate
        rates = track.rates or [rate] * len(track.audio)
        offsets, total = stem_pool_layout(self.lengths(track), hop)
        host = torch.zeros(total, dtype=torch.float32).pin_memory()
        for off, a, r in zip(offsets, track.audio, rates):
            if r == rate:
                host[int(off):int(off) + len(a)] = torch.from_numpy(np.ascontiguousarray(a, np.float32))
        tab = None
        if self.device_labels:
            from mrmt3.labels import note_table
            tab = note_table(track, self._codec.num_velocity_bins)
        if self.cross_track:                 # the track's slot of the arena; whoever had to leave for it leaves both caches
            dev, slot_times, slot_meta = self._arena_slot(track.name, total, len(tab.meta))
            dev.copy_(host, non_blocking=True)
        else:
            dev = host.to(self.device, non_blocking=True)
        for off, a, r, n in zip(offsets, track.audio, rates, self.lengths(track)):
            if r != rate:                    # a stem at its native rate: resampled on the device into its slot, once
                from mrmt3.resample import resample
                y = resample(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device), r, rate)
                assert y.numel() == n
                dev[int(off):int(off) + n] = y
        torch.cuda.current_stream(self.device).synchronize()          # (the pinned buffer is released on return)
        self._pools[track.name] = dev
        if self.cross_track:
            slot_times.copy_(torch.from_numpy(tab.times))
            slot_meta.copy_(torch.from_numpy(tab.meta))
            self._notes[track.name] = (slot_times, slot_meta, tab.n_stems)
        elif self.device_labels:             # the note table travels, counts and leaves with the pool
            self._notes[track.name] = (torch.from_numpy(tab.times).to(self.device), torch.from_numpy(tab.meta).to(self.device),
                                       tab.n_stems)
        self.uploads += 1
        while not self.cross_track and len(self._pools) > 1 and self.cached_bytes() > self.cache_bytes:
            self._notes.pop(self._pools.popitem(last=False)[0], None)
        return dev

    def cached_bytes(self) -> int:
        """Device bytes the cache holds: every track's pool and, with `device_labels`, its note table."""
        return (sum(p.numel() * 4 for p in self._pools.values())
                + sum(t.numel() * 8 + m.numel() * 4 for t, m, _ in self._notes.values()))

    def cached_tracks(self) -> list:
        return list(self._pools)

    def mel(self, track, plan: StemMixPlan) -> torch.Tensor:
        if plan.shift != 0:
            return self._shifted_mel(track, plan)
        start, end, gain, total = self.tables(track, plan)
        pool = self.pool(track)
        assert pool.numel() == total
        return self._sp.logmel_mix(pool, torch.from_numpy(start), torch.from_numpy(end), torch.from_numpy(gain),
                                   self.mel_length, self.cfg, normalize=True,
                                   valid_frames=torch.from_numpy(plan.crops.valid_frames), out_bf16=self.out_bf16)

    def _shifted_mel(self, track, plan: StemMixPlan) -> torch.Tensor:
        """A pitch-shifted plan: one `resample_mix` launch writes the mixed rows, one `logmel` launch transforms them."""
        from mrmt3 import lib
        from mrmt3.resample import device_filter
        pos, begin, end, step, gain, filt, valid, total = self.shifted_tables(track, plan)
        pool = self.pool(track)
        assert pool.numel() == total
        dev = pool.device
        rows = lib.resample_mix(pool, *(torch.from_numpy(t).to(dev) for t in (pos, begin, end, step, gain, filt)),
                                self.mel_length * self.cfg.hop_width, device_filter(plan.step, dev),
                                valid_samples=torch.from_numpy(valid).to(dev))
        return lib.logmel(rows, self._sp.kernel_tables(self.cfg, dev),
                          valid_frames=torch.from_numpy(plan.crops.valid_frames).to(dev), normalize=True,
                          out_bf16=self.out_bf16)

    def prev_windows(self, plan: StemMixPlan) -> np.ndarray:
        """bool [B]: the rows that have a previous window, frames [start - mel_length, start) of their own chunk
        (`Tokenizer.row_targets_prev`); the others carry the placeholder."""
        return plan.crops.start_frame - plan.crops.chunk_start - self.mel_length > 0

    def row_targets_prev(self, track, plan: StemMixPlan):
        """Token ids of every row's previous window on the host (a list of 1-D int arrays, before `pad_targets`)."""
        return [self._host_row(track, plan, b, prev=True) for b in range(len(plan.crops.start_frame))]

    def device_targets(self, track, plan: StemMixPlan):
        """`targets` — and with `with_prev` `targets_prev` — of the plan by ONE launch of the label kernel,
        already padded and on the device.  The previous windows are further rows of the same launch; a row without one has
        an empty stem mask, for which the kernel writes `tie` alone: the placeholder's encoded form.  The status words are
        read back once; a row the kernel could not hold is rebuilt by the host path, and only that row."""
        from mrmt3 import lib
        from mrmt3.labels import keep_masks, tokenizer_frames
        self.pool(track)                                                     # (uploads the note table with the audio)
        times, meta, n_stems = self._notes[track.name]
        B = len(plan.crops.start_frame)
        n = 2 * B if self.with_prev else B
        arg = np.zeros((5, n), np.int64)                                     # keep, start_frame, n_frames, total_frames, scale
        arg[0, :B] = keep_masks(plan.keep).view(np.int64)
        arg[1, :B], arg[2, :B] = plan.crops.start_frame, plan.crops.valid_frames
        if self.with_prev:
            has = self.prev_windows(plan)
            arg[0, B:] = np.where(has, arg[0, :B], 0)
            arg[1, B:], arg[2, B:] = np.where(has, plan.crops.start_frame - self.mel_length, 0), self.mel_length
        arg[3] = tokenizer_frames(self.n_samples(track, plan.step), self.cfg.hop_width)
        arg[4] = np.full(n, float(1 << 32) / float(int(plan.step)), np.float64).view(np.int64)
        raw = np.concatenate([arg.reshape(-1).view(np.uint8), np.full(n, plan.shift, np.int32).view(np.uint8)])
        dev = torch.from_numpy(raw).to(self.device)                          # one copy for the six arrays
        a = dev[:40 * n].view(torch.int64).view(5, n)
        tg, status = lib.label_rows(times, meta, n_stems, a[0], a[1], a[2], a[3], a[4].view(torch.float64),
                                    dev[40 * n:].view(torch.int32), self._codec, self.event_length)
        bad = np.nonzero(status.cpu().numpy())[0]
        if len(bad):
            self.host_label_rows += len(bad)
            fixed = pad_targets([self._host_row(track, plan, int(b) % B, prev=b >= B) for b in bad], self.event_length)
            tg[torch.from_numpy(bad).to(self.device)] = fixed.to(self.device)
        return (tg[:B], tg[B:]) if self.with_prev else (tg,)

    def build(self, track, plan=None, partners=()):
        """`(mel, targets)`; `(mel, targets, targets_prev)` with `with_prev`.  `partners` (tracks, at most 3; needs
        `cross_track`) may also stand in `plan`'s place: `build(track, partners)`.  With `cross_track` or `per_row_shift`
        the rows are those of `plan_cross` (or of the `CrossMixPlan` given)."""
        if isinstance(plan, (list, tuple)):
            plan, partners = None, plan
        if self.cross_track or self.per_row_shift or isinstance(plan, CrossMixPlan):
            plan = plan or self.plan_cross(track, partners)
            return (self.cross_mel(plan),) + self.cross_targets(plan)
        if len(partners):
            raise ValueError("partners need cross_track=True")
        plan = plan or self.plan(track)
        mel = self.mel(track, plan)
        if self.device_labels:
            return (mel,) + self.device_targets(track, plan)
        tg = pad_targets(self.row_targets(track, plan), self.event_length)
        return mel, tg.to(self.device, non_blocking=True)

    # ---- cross-track rows and per-row shifts ----------------------------------------------------------
    def plan_cross(self, track, partners=()) -> CrossMixPlan:
        """Rows of virtual tracks over `track` and up to 3 `partners` (a ValueError beyond that, and for more than 64 stems
        in all).  The rng is consumed in this order:
          1. the draws of `plan_stem_mix` over the UNSHIFTED visited track, unchanged (no plan-level shift is drawn);
          2. then row by row:
             (a) with `per_row_shift` and `pitch_shift` = S > 0 one `randint(-S, S)`: part 0's shift, clamped into
                 `shift_range(track)`;
             (b) for each partner in the given order one `random()`: the partner takes part iff it is < cross_prob, and
                 then draws its shift as in (a) into its own range, one `randint(0, max(0, frames - mel_length))` for its
                 start in its own stretched frames, one `random()` per stem in stem order — the stem is borrowed iff the
                 draw is < keep_prob and its (program, is_drum) is not kept in another part of the row already; the draw
                 is made either way —, then one `uniform(-gain_db, gain_db)` per borrowed stem.  A partner without a
                 borrowed stem is no part.
        Part 0 starts at g_0 = min(floor(start_frame * 2^32 / step_0), frames_0 - 1) of its stretched frames, `chunk_start`
        is mapped the same way, n_frames = min(valid_frames, frames_0 - g_0).  `is_deterministic` ignores partners and
        shifts: the rows are `plan`'s."""
        from mrmt3.resample import ratio_step
        from mrmt3.stems import shift_range
        partners = list(partners)
        if partners and not self.cross_track:
            raise ValueError("partners need cross_track=True")
        if len(partners) > MAX_PARTS - 1:
            raise ValueError("a row has at most %d parts: %d partners given" % (MAX_PARTS, len(partners)))
        tracks = [track] + ([] if self.is_deterministic else partners)
        if sum(len(t.audio) for t in tracks) > MAX_SOURCES:
            raise ValueError("%d stems in the visited track and its partners, a row takes %d sources"
                             % (sum(len(t.audio) for t in tracks), MAX_SOURCES))
        rng = self.rng or _random
        base = plan_stem_mix(self.n_frames(track), len(track.audio), self.mel_length, self.num_rows, self.split_len,
                             self.keep_prob, self.min_stems, self.gain_db, self.is_deterministic, self.rng)
        B, T = len(base.crops.start_frame), len(tracks)
        part = np.zeros((B, T), bool)
        part[:, 0] = True
        keep = [base.keep] + [np.zeros((B, len(t.audio)), bool) for t in tracks[1:]]
        gain = [base.gain] + [np.zeros((B, len(t.audio)), np.float32) for t in tracks[1:]]
        shift, step = np.zeros((B, T), np.int32), np.full((B, T), 1 << 32, np.int64)
        start = np.zeros((B, T), np.int64)
        start[:, 0] = base.crops.start_frame
        chunk, n_frames = base.crops.chunk_start.copy(), base.crops.valid_frames.astype(np.int32)
        shifting = self.per_row_shift and self.pitch_shift > 0 and not self.is_deterministic

        ranges = [shift_range(t) for t in tracks] if shifting else None      # (a scan of the track's notes: once, not per draw)

        def draw_shift(t):
            lo, hi = ranges[t]
            k = max(lo, min(hi, int(rng.randint(-self.pitch_shift, self.pitch_shift))))
            return k, (1 << 32 if k == 0 else ratio_step(2.0 ** (k / 12.0)))

        for b in range(B if not self.is_deterministic else 0):
            if shifting:
                shift[b, 0], step[b, 0] = draw_shift(0)
            frames = self.n_frames(track, int(step[b, 0]))
            to_stretched = lambda f: min((int(f) << 32) // int(step[b, 0]), frames - 1)
            start[b, 0], chunk[b] = to_stretched(base.crops.start_frame[b]), to_stretched(base.crops.chunk_start[b])
            n_frames[b] = min(int(base.crops.valid_frames[b]), frames - int(start[b, 0]))
            taken = {track.programs[s] for s in np.nonzero(keep[0][b])[0]}
            for t in range(1, T):
                if not rng.random() < self.cross_prob:
                    continue
                tr = tracks[t]
                if shifting:
                    shift[b, t], step[b, t] = draw_shift(t)
                start[b, t] = rng.randint(0, max(0, self.n_frames(tr, int(step[b, t])) - self.mel_length))
                mine = set()
                for s in range(len(tr.audio)):
                    pair = (int(tr.programs[s][0]), bool(tr.programs[s][1]))
                    if rng.random() < self.keep_prob and pair not in taken:
                        keep[t][b, s] = True
                        mine.add(pair)
                for s in np.nonzero(keep[t][b])[0]:
                    gain[t][b, s] = np.float32(10.0 ** (rng.uniform(-self.gain_db, self.gain_db) / 20.0))
                part[b, t] = bool(keep[t][b].any())
                if part[b, t]:
                    taken |= mine
                else:
                    shift[b, t], step[b, t], start[b, t] = 0, 1 << 32, 0
        return CrossMixPlan(tracks, base, part, keep, gain, shift, step, start, chunk, n_frames)

    def _layout(self, plan: CrossMixPlan, bases=None):
        lengths = [self.lengths(t) for t in plan.tracks]
        if bases is None:                    # tracks end to end, each as `stem_pool_layout` lays it (the host's own layout)
            totals = [stem_pool_layout(n, self.cfg.hop_width)[1] for n in lengths]
            bases = np.concatenate([[0], np.cumsum(totals)[:-1]]).astype(np.int64)
        return bases, lengths

    def cross_tables(self, plan: CrossMixPlan, bases=None, pool_samples: int | None = None):
        """The audio tables of a cross plan on the host, checked: `cross_resample_tables` (8 entries) when any row is
        shifted, else `cross_mix_tables` (3 entries).  bases: where every track of the plan starts in the one pool of
        `pool_samples` samples (default: the tracks end to end)."""
        from mrmt3.resample import check_resample_tables
        hop = self.cfg.hop_width
        bases, lengths = self._layout(plan, bases)
        if pool_samples is None:
            pool_samples = int(bases[-1]) + stem_pool_layout(lengths[-1], hop)[1]
        if plan.any_shift:
            tabs = cross_resample_tables(plan, bases, lengths, hop)
            check_resample_tables(*tabs[:6], pool_samples, max(1, len(tabs[7])))
        else:
            tabs = cross_mix_tables(plan, bases, lengths, hop)
            check_mix_tables(*tabs, pool_samples, hop)
        return tabs

    def _arena_slot(self, name, samples: int, notes: int):
        """The arena views of a new track (audio, note times, note meta); tracks evicted for it leave every cache."""
        if self._arena is None:
            note_cap = max(1, self.cache_bytes // 32 // 24)                       # 24 bytes a note: 1/32 of the cache
            audio_cap = max(0, self.cache_bytes - 24 * note_cap) // 4
            self._arena = (TrackArena(audio_cap, note_cap), torch.empty(audio_cap, dtype=torch.float32, device=self.device),
                           torch.zeros(note_cap, 2, dtype=torch.float64, device=self.device),
                           torch.zeros(note_cap, 4, dtype=torch.int32, device=self.device))
        where, audio, times, meta = self._arena
        for gone in where.place(name, samples, notes, set(self._in_use) | {name}):
            self._pools.pop(gone, None)
            self._notes.pop(gone, None)
        (a, n), (f, c) = where.slots[name]
        return audio[a:a + n], times[f:f + c], meta[f:f + c]

    def _resident(self, plan: CrossMixPlan):
        """Every track of the plan on the device at once -> (the one pool, bases [T], note times, note meta, first [T],
        count [T]).  Without `cross_track` the plan has one track and the pool is that track's."""
        self._in_use = tuple(t.name for t in plan.tracks)
        try:
            for t in plan.tracks:
                self.pool(t)
        finally:
            self._in_use = ()
        if self._arena is None:
            times, meta, _ = self._notes[plan.tracks[0].name]
            return self._pools[plan.tracks[0].name], np.zeros(1, np.int64), times, meta, [0], [meta.shape[0]]
        where, audio, times, meta = self._arena
        slots = [where.slots[t.name] for t in plan.tracks]
        return (audio, np.array([s[0][0] for s in slots], np.int64), times, meta, [s[1][0] for s in slots],
                [s[1][1] for s in slots])

    def _filter_stack(self, steps):
        """`stack_filters` over the tables of `steps` on the device, cached per set of steps."""
        from fractions import Fraction
        from mrmt3.resample import resample_filter, stack_filters
        key = tuple(steps)
        if key in self._filters:
            self._filters.move_to_end(key)
            return self._filters[key]
        tabs = stack_filters([resample_filter(Fraction(int(st), 1 << 32)) for st in steps])
        self._filters[key] = torch.from_numpy(tabs).to(self.device)
        while len(self._filters) > 16:
            self._filters.popitem(last=False)
        return self._filters[key]

    def cross_mel(self, plan: CrossMixPlan) -> torch.Tensor:
        """One `logmel_mix` launch for a plan without any shift; else one `resample_mix` and one `logmel` launch."""
        from mrmt3 import lib
        if self.device.type != "cuda":
            raise RuntimeError("StemMixBatcher builds batches on the GPU (no CPU fallback)")
        pool, bases = self._resident(plan)[:2]
        tabs = self.cross_tables(plan, bases, pool.numel())
        dev = pool.device
        vf = torch.from_numpy(plan.n_frames.astype(np.int32))
        if not plan.any_shift:
            start, end, gain = tabs
            return self._sp.logmel_mix(pool, torch.from_numpy(start), torch.from_numpy(end), torch.from_numpy(gain),
                                       self.mel_length, self.cfg, normalize=True, valid_frames=vf, out_bf16=self.out_bf16)
        rows = lib.resample_mix(pool, *(torch.from_numpy(t).to(dev) for t in tabs[:6]), self.mel_length * self.cfg.hop_width,
                                self._filter_stack(tabs[7]), valid_samples=torch.from_numpy(tabs[6]).to(dev))
        return lib.logmel(rows, self._sp.kernel_tables(self.cfg, dev), valid_frames=vf.to(dev), normalize=True,
                          out_bf16=self.out_bf16)

    def cross_prev_windows(self, plan: CrossMixPlan) -> np.ndarray:
        """bool [B]: the has-previous rule on part 0's stretched start and chunk start."""
        return plan.start[:, 0] - plan.chunk_start - self.mel_length > 0

    def virtual_parts(self, plan: CrossMixPlan, b: int) -> list:
        """Row b's parts as the definition takes them (`mrmt3.stems.virtual_note_sequence`)."""
        from mrmt3.stems import VirtualPart
        delay = plan.delay
        return [VirtualPart(tr, tuple(int(s) for s in np.nonzero(plan.keep[t][b])[0]), int(plan.shift[b, t]),
                            int(plan.step[b, t]), int(delay[b, t]))
                for t, tr in enumerate(plan.tracks) if plan.part[b, t]]

    def cross_host_row(self, plan: CrossMixPlan, b: int, prev: bool = False):
        """Token ids of row b, or of its previous window, from the definition: one tokenisation of the virtual track."""
        from mrmt3.stems import virtual_n_samples, virtual_note_sequence
        if prev and not self.cross_prev_windows(plan)[b]:
            return self.tokenizer.row_targets_prev(None, 0, 0, self.mel_length)          # the placeholder
        parts = self.virtual_parts(plan, b)
        ns = virtual_note_sequence(parts, self.cfg.sample_rate, self.cfg.hop_width)
        if not ns.notes:
            return np.array([self.tokenizer.tie_token], np.int64)
        feats = self.tokenizer.tokenize(ns, virtual_n_samples(parts, self.cfg.sample_rate, self.cfg.hop_width))
        F = int(plan.start_frame[b])
        if prev:
            return self.tokenizer.row_targets(feats, F - self.mel_length, self.mel_length)
        return self.tokenizer.row_targets(feats, F, int(plan.n_frames[b]))

    def cross_label_arrays(self, plan: CrossMixPlan, first, count):
        """The per-(row, part) and per-row arguments of `mrmt3_label_rows_parts_fwd` for the plan, the previous windows as
        further rows when `with_prev`: (note_first, note_count int32, keep uint64, delay int64, scale float64, shift int32
        [n, P]; start_frame, n_frames, total_frames int64 [n]).  first / count: every track's table in the note arena."""
        from mrmt3.labels import keep_masks, tokenizer_frames
        hop = self.cfg.hop_width
        B, T = plan.part.shape
        P = int(plan.part.sum(axis=1).max())
        nf, nc, sh = (np.zeros((B, P), np.int32) for _ in range(3))
        kp, dl, sc = np.zeros((B, P), np.uint64), np.zeros((B, P), np.int64), np.ones((B, P), np.float64)
        total = np.zeros(B, np.int64)
        delay, masks = plan.delay, [keep_masks(k) for k in plan.keep]
        for b in range(B):
            n_samples = 0
            for p, t in enumerate(np.nonzero(plan.part[b])[0]):
                nf[b, p], nc[b, p], kp[b, p] = first[t], count[t], masks[t][b]
                dl[b, p], sh[b, p] = delay[b, t], plan.shift[b, t]
                sc[b, p] = float(1 << 32) / float(int(plan.step[b, t]))
                n_samples = max(n_samples, self.n_samples(plan.tracks[t], int(plan.step[b, t])) + int(delay[b, t]) * hop)
            total[b] = tokenizer_frames(n_samples, hop)
        f0, n = plan.start_frame.astype(np.int64), plan.n_frames.astype(np.int64)
        if self.with_prev:
            has = self.cross_prev_windows(plan)
            nf, nc, dl, sc, sh = (np.concatenate([a, a]) for a in (nf, nc, dl, sc, sh))
            kp = np.concatenate([kp, np.where(has[:, None], kp, np.uint64(0))])
            f0 = np.concatenate([f0, np.where(has, f0 - self.mel_length, 0)])
            n = np.concatenate([n, np.full(B, self.mel_length, np.int64)])
            total = np.concatenate([total, total])
        return nf, nc, kp, dl, sc, sh, f0, n, total

    def cross_targets(self, plan: CrossMixPlan):
        """`targets` — and with `with_prev` `targets_prev` — of a cross plan by ONE launch of `mrmt3_label_rows_parts_fwd`
        over the note arena.  A row the kernel reports (status != 0: a shared pair, a capacity, an order) is rebuilt from
        the definition on the host, and only that row."""
        from mrmt3 import lib
        _, _, times, meta, first, count = self._resident(plan)
        arrays = self.cross_label_arrays(plan, first, count)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64 else a)).to(self.device)
        tg, status = lib.label_rows_parts(times, meta, *(up(a) for a in arrays), self._codec, self.event_length)
        B = len(plan.n_frames)
        bad = np.nonzero(status.cpu().numpy())[0]
        if len(bad):
            self.host_label_rows += len(bad)
            fixed = pad_targets([self.cross_host_row(plan, int(b) % B, prev=b >= B) for b in bad], self.event_length)
            tg[torch.from_numpy(bad).to(self.device)] = fixed.to(self.device)
        return (tg[:B], tg[B:]) if self.with_prev else (tg,)

# ---- cross-track rows and per-row shifts -----------------------------------------------------------------------

MAX_PARTS = 4                    # parts of one row: the visited track and up to 3 partners (LB_MAX_PARTS)
MAX_SOURCES = 64                 # stems of all tracks of one plan: the audio kernels' sources per row


@dataclass
class CrossMixPlan:
    """Rows of virtual tracks.  `tracks` = [visited track] + partners; track t is a part of row b iff part[b, t] (track 0
    always is), played at step[b, t] / 2^32 times its speed (shift[b, t] semitones) from frame start[b, t] of its own
    stretched frames.  keep[t] / gain[t] are [B, S_t] like `StemMixPlan`'s, all False / 0 where the track is no part."""
    tracks: list
    base: StemMixPlan            # the plan of the unshifted visited track the rows were derived from
    part: np.ndarray             # bool [B, T]
    keep: list                   # T x bool [B, S_t]
    gain: list                   # T x float32 [B, S_t]
    shift: np.ndarray            # int32 [B, T]
    step: np.ndarray             # int64 [B, T]
    start: np.ndarray            # int64 [B, T]   g_p
    chunk_start: np.ndarray      # int64 [B]      of track 0, in its stretched frames
    n_frames: np.ndarray         # int32 [B]

    @property
    def start_frame(self) -> np.ndarray:
        """F [B]: the row's start in the virtual track's frames, the largest start of its parts."""
        return np.where(self.part, self.start, 0).max(axis=1)

    @property
    def delay(self) -> np.ndarray:
        """int64 [B, T]: F - g_p, 0 where the track is no part."""
        return np.where(self.part, self.start_frame[:, None] - self.start, 0)

    @property
    def any_shift(self) -> bool:
        return bool((self.shift != 0).any())


class TrackArena:
    """Where the cached tracks lie in the two arenas (host bookkeeping only): every track one slot of `audio` samples and
    one of `notes` notes, first fit.  A track that does not fit evicts the least recently used tracks that are not in use
    until it does; one that cannot fit at all is a ValueError."""

    def __init__(self, audio_capacity: int, note_capacity: int):
        from collections import OrderedDict
        self.capacity = (int(audio_capacity), int(note_capacity))
        self.slots = OrderedDict()           # name -> ((audio offset, samples), (first note, notes)), least recent first

    def touch(self, name) -> None:
        self.slots.move_to_end(name)

    def _fit(self, which: int, size: int):
        at = 0
        for off, n in sorted(s[which] for s in self.slots.values()):
            if off - at >= size:
                return at
            at = off + n
        return at if self.capacity[which] - at >= size else None

    def place(self, name, samples: int, notes: int, in_use=()) -> list:
        """Give `name` its slots; returns the names evicted for it, in eviction order."""
        evicted = []
        while True:
            at = self._fit(0, samples), self._fit(1, notes)
            if at[0] is not None and at[1] is not None:
                self.slots[name] = ((at[0], int(samples)), (at[1], int(notes)))
                return evicted
            victim = next((n for n in self.slots if n not in in_use), None)
            if victim is None:
                raise ValueError("track %s (%d samples, %d notes) does not fit the arena of %d samples and %d notes beside "
                                 "the %d tracks in use" % (name, samples, notes, *self.capacity, len(self.slots)))
            del self.slots[victim]
            evicted.append(victim)


def cross_sources(plan: CrossMixPlan, bases, lengths, hop: int):
    """Per source of a plan — every stem of every track, track after track — over one pool in which track t's stems lie
    from sample bases[t] on as `stem_pool_layout` lays them: (begin, end int64 [K] of the stem, track index [K], stem
    index [K]).  lengths: T lists of stem lengths in samples."""
    begin, end, tr, st = [], [], [], []
    for t, (base, lens) in enumerate(zip(bases, lengths)):
        offsets, _ = stem_pool_layout(lens, hop)
        for s, (off, n) in enumerate(zip(offsets, lens)):
            begin.append(int(base) + int(off))
            end.append(int(base) + int(off) + int(n))
            tr.append(t)
            st.append(s)
    return np.array(begin, np.int64), np.array(end, np.int64), np.array(tr), np.array(st)


def cross_resample_tables(plan: CrossMixPlan, bases, lengths, hop: int):
    """The resampler's tables of a cross plan (any row shifted): (src_pos, src_begin, src_end, src_step int64 [B, K],
    src_gain float32 [B, K], src_filt int32 [B, K], valid_samples int64 [B], steps) — `steps` the distinct steps other
    than 1 in ascending order, src_filt a source's index among them, -1 (pass-through) at step 1.  Source (t, s) of row b
    starts at (begin << 32) + start[b, t] * hop * step[b, t], bounded by its own stem; gain 0 for a stem that is not kept
    and, as in `resample_tables`, for a crop that starts at or behind the stretched stem's end."""
    from mrmt3.resample import out_length
    begin, end, tr, st = cross_sources(plan, bases, lengths, hop)
    B, K = len(plan.n_frames), len(begin)
    steps = sorted(set(int(v) for v in plan.step[plan.part]) - {1 << 32})
    shape = (B, K)
    pos, step = np.zeros(shape, np.int64), np.full(shape, 1 << 32, np.int64)
    gain, filt = np.zeros(shape, np.float32), np.full(shape, -1, np.int32)
    for b in range(B):
        for k in range(K):
            t, s = int(tr[k]), int(st[k])
            pos[b, k] = int(begin[k]) << 32
            if not (plan.part[b, t] and plan.keep[t][b, s]):
                continue
            sp = int(plan.step[b, t])
            first = int(plan.start[b, t]) * hop                                   # in stretched samples
            n = int(end[k] - begin[k])
            if first >= (n if sp == 1 << 32 else out_length(n, sp)):
                continue
            pos[b, k] += first * sp
            step[b, k], gain[b, k] = sp, plan.gain[t][b, s]
            filt[b, k] = -1 if sp == 1 << 32 else steps.index(sp)
    return (pos, np.broadcast_to(begin, shape).copy(), np.broadcast_to(end, shape).copy(), step, gain, filt,
            plan.n_frames.astype(np.int64) * hop, steps)


def cross_mix_tables(plan: CrossMixPlan, bases, lengths, hop: int):
    """The log-mel mix kernel's tables of a cross plan without any shift: (start_frames, src_end int64 [B, K], src_gain
    float32 [B, K]) as `mix_tables` makes them, every track at its own start."""
    if plan.any_shift:
        raise ValueError("cross_mix_tables: the plan has shifted rows, they go through cross_resample_tables")
    begin, end, tr, st = cross_sources(plan, bases, lengths, hop)
    B, K = len(plan.n_frames), len(begin)
    start = begin[None, :] // hop + np.where(plan.part, plan.start, 0)[:, tr]
    endb = np.broadcast_to(end, (B, K)).copy()
    gain = np.stack([np.where(plan.part[:, t] & plan.keep[t][:, s], plan.gain[t][:, s], np.float32(0))
                     for t, s in zip(tr, st)], axis=1).astype(np.float32)
    over = start * hop >= endb
    return np.where(over, endb // hop, start).astype(np.int64), endb, np.ascontiguousarray(np.where(over, np.float32(0), gain))
