"""Multi-stem tracks for stem-mix training: a folder of tracks, each a set of stems with their own MIDI.

A track is a directory with `stems/<name>.wav` (mono, the config's sample rate — or, with `any_rate=True`, any rate from a
quarter to four times that: the batcher resamples such a stem on the device when it uploads the track) and
`MIDI/<name>.mid` (read with `contrib.midi_io`) — the layout of a Slakh track after resampling and WAV conversion.  A
stem's program and drum flag come from its MIDI file (the first instrument that has notes); an optional `programs.json`
next to the two directories, `{name: {"program": int, "is_drum": bool}}`, overrides them.  Nothing here knows an
instrument-class table: the programs are whatever the files say.

`merged_note_sequence(track, kept)` is the DEFINITION of a mixed row's label: the notes of exactly the kept stems, the
instrument index a stem's place among the kept ones, the length the track's.  `mrmt3.batching.StemMixBatcher` tokenises
that sequence with `mrmt3.tokenizer.Tokenizer`.  `speed_note_sequence(ns, shift, step)` is the DEFINITION of the label of a
pitch-shifted row: the track played at step / 2^32 times its speed.  Host code (numpy); no third-party dataset package.
"""
from __future__ import annotations

import dataclasses
import json
import os
import random as _random

import numpy as np

from contrib import audio_io, midi_io
from contrib.note_sequences import Note, NoteSequence


@dataclasses.dataclass
class StemTrack:
    name: str                    # the track directory (the device cache's key)
    stem_names: list             # [S] file stems, sorted
    audio: list                  # [S] float32 [n_s] mono samples, unequal lengths allowed
    notes: list                  # [S] NoteSequence of the stem alone (program / is_drum set on every note)
    programs: list               # [S] (program, is_drum)
    rates: list | None = None    # [S] sample rate of each stem's audio; None: every stem is at the config's rate

    def lengths(self, sample_rate: int = 16000) -> list:
        """Samples of every stem at `sample_rate`: its own length, or what `mrmt3.resample.resample` makes of it."""
        if self.rates is None:
            return [len(a) for a in self.audio]
        from fractions import Fraction
        from mrmt3.resample import out_length, ratio_step
        return [len(a) if r == sample_rate else out_length(len(a), ratio_step(Fraction(int(r), int(sample_rate))))
                for a, r in zip(self.audio, self.rates)]

    @property
    def n_samples(self) -> int:
        """The track's length: its longest stem (at 16 kHz; `max(track.lengths(rate))` for another config)."""
        return max(self.lengths())

    @property
    def total_time(self) -> float:
        return max([ns.total_time for ns in self.notes] + [0.0])


def merged_note_sequence(track: StemTrack, kept) -> NoteSequence:
    """The NoteSequence of the sub-mix `kept` (stem indices, ascending): exactly those stems' notes (copies), stem after
    stem, instrument = the stem's index among the kept ones, total_time = the whole track's."""
    out = NoteSequence(total_time=track.total_time)
    for j, s in enumerate(kept):
        for n in track.notes[s].notes:
            out.notes.append(dataclasses.replace(n, instrument=j))
    return out


def speed_note_sequence(ns: NoteSequence, shift: int, step: int) -> NoteSequence:
    """`ns` played at step / 2^32 times its speed (32.32 fixed point, `mrmt3.resample.ratio_step(2 ** (shift / 12))`):
    every start and end time and total_time multiplied by 2^32 / step in float64, every note that is not a drum note
    transposed by `shift` semitones (drum notes keep their pitch: it names the instrument).  Copies; `ns` is untouched."""
    scale = float(1 << 32) / float(int(step))
    out = NoteSequence(total_time=ns.total_time * scale, ticks_per_quarter=ns.ticks_per_quarter)
    for n in ns.notes:
        out.notes.append(dataclasses.replace(n, start_time=n.start_time * scale, end_time=n.end_time * scale,
                                             pitch=n.pitch if n.is_drum else n.pitch + int(shift)))
    return out


@dataclasses.dataclass
class VirtualPart:
    """One part of a cross-track row: the stems `kept` (indices, ascending) of `track`, played at
    step / 2^32 times its speed and transposed by `shift` semitones, then delayed by `delay_frames` whole frames."""
    track: StemTrack
    kept: tuple
    shift: int = 0
    step: int = 1 << 32
    delay_frames: int = 0


def _stretched_samples(track: StemTrack, step: int, sample_rate: int) -> int:
    from mrmt3.resample import out_length
    return max(n if step == 1 << 32 else out_length(n, step) for n in track.lengths(sample_rate))


def virtual_n_samples(parts, sample_rate: int = 16000, hop: int = 128) -> int:
    """The virtual track's length in samples: the longest (stretched) part behind its delay."""
    return max(_stretched_samples(p.track, int(p.step), sample_rate) + int(p.delay_frames) * hop for p in parts)


def virtual_note_sequence(parts, sample_rate: int = 16000, hop: int = 128) -> NoteSequence:
    """The DEFINITION of a cross-track row's label: the notes of every part in part order, each part
    `speed_note_sequence(merged_note_sequence(track, kept), shift, step)` (untouched when shift == 0) with
    fl(delay_frames / fps) added to every start and end — one f64 rounding for the quotient, one for the sum, and no
    change at all when delay_frames == 0.  fps = sample_rate / hop.  The sequence is tokenised at `virtual_n_samples`."""
    fps = float(sample_rate) / float(hop)
    out = NoteSequence()
    for p in parts:
        ns = merged_note_sequence(p.track, tuple(p.kept))
        if int(p.shift) != 0:
            ns = speed_note_sequence(ns, int(p.shift), int(p.step))
        delay = float(int(p.delay_frames)) / fps
        for n in ns.notes:
            if int(p.delay_frames) != 0:
                n = dataclasses.replace(n, start_time=n.start_time + delay, end_time=n.end_time + delay)
            out.notes.append(n)
        out.total_time = max(out.total_time, ns.total_time + delay)
    return out


def shift_range(track: StemTrack):
    """(lowest, highest) pitch shift in semitones that keeps every non-drum note of the track inside the codec's 0..127:
    (-min_pitch, 127 - max_pitch); (-127, 127) for a track without pitched notes.  A function of the track alone."""
    pitches = [n.pitch for ns in track.notes for n in ns.notes if not n.is_drum]
    return (-min(pitches), 127 - max(pitches)) if pitches else (-127, 127)


def load_track(path: str, sample_rate: int = 16000, any_rate: bool = False) -> StemTrack:
    stem_dir, midi_dir = os.path.join(path, "stems"), os.path.join(path, "MIDI")
    names = sorted(f[:-4] for f in os.listdir(stem_dir) if f.lower().endswith(".wav"))
    if not names:
        raise ValueError(f"{stem_dir}: no .wav stems")
    override = {}
    if os.path.exists(os.path.join(path, "programs.json")):
        with open(os.path.join(path, "programs.json")) as f:
            override = json.load(f)
    audio, notes, programs, rates = [], [], [], []
    for name in names:
        wav, mid = os.path.join(stem_dir, name + ".wav"), os.path.join(midi_dir, name + ".mid")
        x, rate = audio_io.read_wav(wav)
        if rate != sample_rate and not any_rate:
            raise ValueError(f"{wav}: sample rate {rate}, the config's is {sample_rate} (resample the stems first)")
        if not sample_rate <= 4 * rate <= 16 * sample_rate:
            raise ValueError(f"{wav}: sample rate {rate} is outside 1/4 to 4 times the config's {sample_rate}")
        if not os.path.exists(mid):
            raise ValueError(f"{wav}: the stem has no MIDI file ({mid} is missing)")
        midi = midi_io.read_midi(mid)
        first = next((i for i in midi.instruments if i.notes), None)
        program, is_drum = (first.program, first.is_drum) if first is not None else (0, False)
        if name in override:
            program = int(override[name].get("program", program))
            is_drum = bool(override[name].get("is_drum", is_drum))
        ns = NoteSequence(ticks_per_quarter=midi.resolution)
        for inst in midi.instruments:
            for n in inst.notes:
                ns.notes.append(Note(n.start, n.end, n.pitch, n.velocity, program, is_drum, 0))
                ns.total_time = max(ns.total_time, n.end)
        audio.append(x)
        notes.append(ns)
        programs.append((program, is_drum))
        rates.append(int(rate))
    return StemTrack(path, names, audio, notes, programs, rates if any(r != sample_rate for r in rates) else None)


def load_stem_folder(root: str, sample_rate: int = 16000, any_rate: bool = False) -> list:
    """Every track directory under `root` (one that holds `stems/`), in name order."""
    dirs = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d, "stems")))
    if not dirs:
        raise ValueError(f"{root}: no track directories (a track holds stems/<name>.wav and MIDI/<name>.mid)")
    return [load_track(os.path.join(root, d), sample_rate, any_rate) for d in dirs]


def epoch_order(n_tracks: int, seed: int, epoch: int) -> list:
    """The order in which an epoch visits the tracks: a function of (seed, epoch) alone, the same on every rank."""
    order = list(range(n_tracks))
    _random.Random(int(seed) * 1000003 + int(epoch)).shuffle(order)
    return order


def rank_shard(order: list, rank: int, world: int) -> list:
    """Rank `rank`'s tracks of an epoch: every world-th entry of the order.  The shards are disjoint; the order is cut to
    a multiple of `world` first so that every rank takes the same number of steps (at most world - 1 tracks wait for an
    epoch whose order places them earlier)."""
    if world > 1:
        order = order[:len(order) // world * world]
    return order[rank::world]
