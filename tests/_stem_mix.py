"""The stem-mix contract of include/mrmt3_hip.h (mrmt3_logmel_mix_fwd) restated, and the constructions the stem-mix tests
share (tests/test_stem_mix_cpu.py, tests/test_stem_mix_gpu.py).  numpy only at import; nothing here touches the library.

`mix_rows` is the contract, not the kernels: row b, sample i = the f32 sum, in source order, of fl(gain * sample) over
the sources that contribute at i — gain != 0, 0 <= start < min(end, pool_samples), start + i < that end, and
i < valid_frames[b] * hop.  The product is rounded to f32 before it is added (numpy rounds every f32 operation: there is
no fused multiply-add to be had), the sum starts from +0.
"""
import numpy as np

F32 = np.float32
GAINS = (1.0, -0.5, 10.0 ** (6.0 / 20.0), 10.0 ** (-6.0 / 20.0), 0.75)


def mix_rows(pool, start, end, gain, n_samples, hop, valid_frames=None):
    """float32 [B, n_samples].  pool float32 [P]; start / end int64 [B, K] pool offsets; gain float32 [B, K]."""
    pool = np.asarray(pool, F32)
    start, end, gain = np.asarray(start, np.int64), np.asarray(end, np.int64), np.asarray(gain, F32)
    B, K = gain.shape
    rows = np.zeros((B, n_samples), F32)
    for b in range(B):
        lim = n_samples if valid_frames is None else min(n_samples, int(valid_frames[b]) * hop)
        acc = rows[b]
        for k in range(K):
            g = gain[b, k]
            if g == 0:
                continue                                     # not read at all: start and end are ignored
            st, en = int(start[b, k]), min(int(end[b, k]), len(pool))
            if st < 0 or st >= en:
                continue
            cnt = min(en - st, lim)
            if cnt <= 0:
                continue
            prod = (g * pool[st:st + cnt]).astype(F32)       # f32 x f32 -> f32, rounded once
            acc[:cnt] = (acc[:cnt] + prod).astype(F32)
    return rows


def mix_rows_f64(pool, start, end, gain, n_samples, hop, valid_frames=None):
    """The same sum in float64 and the per-sample magnitude sum_k |g_k s_k|: (rows, mag), both [B, n_samples]."""
    pool64 = np.asarray(pool, F32).astype(np.float64)
    B, K = np.asarray(gain).shape
    rows, mag = np.zeros((B, n_samples)), np.zeros((B, n_samples))
    for b in range(B):
        lim = n_samples if valid_frames is None else min(n_samples, int(valid_frames[b]) * hop)
        for k in range(K):
            g = float(F32(gain[b][k]))
            st, en = int(start[b][k]), min(int(end[b][k]), len(pool64))
            if g == 0 or st < 0 or st >= en or min(en - st, lim) <= 0:
                continue
            cnt = min(en - st, lim)
            rows[b, :cnt] += g * pool64[st:st + cnt]
            mag[b, :cnt] += np.abs(g * pool64[st:st + cnt])
    return rows, mag


def stem_case(n_src, n_samples, hop=128, seed=0, amp=1.0):
    """Three rows of `n_src` sources over one pool whose stems lie end to end behind odd-sized NaN gaps (what no source
    may read is NaN).  Row 0: source 0 ends INSIDE the crop, (with 5 sources) source 3 has gain 0 and points at a gap.
    Row 1: its last source ends exactly on a frame edge, and valid_frames is short.  Row 2: every source is silent past
    sample 0 (its stem ends one sample behind the crop's start).  Gains run through 1, -0.5, 10^(+-6/20), 0.75.
    Returns dict(pool, start, end, gain, valid_frames, n_samples, hop)."""
    rs = np.random.RandomState(1000 * n_src + n_samples % 997 + seed)
    F = -(-n_samples // hop)
    B = 3
    pieces, start, end = [], np.zeros((B, n_src), np.int64), np.zeros((B, n_src), np.int64)
    gain = np.zeros((B, n_src), F32)
    pos = 0
    for b in range(B):
        for k in range(n_src):
            lead = int(rs.randint(0, 300))                   # samples of the stem before the crop's start
            avail = n_samples + int(rs.randint(1, 500))      # samples of the stem from the crop's start on
            if b == 0 and k == 0:
                avail = n_samples // 2 + 3
            if b == 1 and k == n_src - 1:
                avail = hop * max(1, F // 3)                 # (before valid_frames[1] * hop = hop * (F // 2))
            if b == 2:
                avail = 1
            gap = 2 * int(rs.randint(3, 40)) + 1
            pieces.append(np.full(gap, np.nan, F32))
            pos += gap
            pieces.append((rs.uniform(-1, 1, lead + avail) * amp * 2.0 ** -(k % 3)).astype(F32))
            start[b, k], end[b, k] = pos + lead, pos + lead + avail
            pos += lead + avail
            gain[b, k] = F32(GAINS[(b + k) % len(GAINS)])
    pieces.append(np.full(9, np.nan, F32))
    pool = np.concatenate(pieces)
    if n_src >= 5:
        gain[0, 3] = 0
        start[0, 3], end[0, 3] = 1, 8                        # inside the first NaN gap: must not be read
    vf = np.array([F, max(1, F // 2), F], np.int32)
    return dict(pool=pool, start=start, end=end, gain=gain, valid_frames=vf, n_samples=n_samples, hop=hop)


def synthetic_tracks(n_tracks=2, seconds=(5.0, 3.5, 4.25), seed=7, sample_rate=16000):
    """`n_tracks` in-memory `mrmt3.stems.StemTrack`s of three stems of unequal lengths; stem 1 is a drum stem."""
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.stems import StemTrack
    rs = np.random.RandomState(seed)
    tracks = []
    for t in range(n_tracks):
        audio, notes, programs = [], [], []
        for s, sec in enumerate(seconds):
            n = int((sec + 0.3 * t) * sample_rate) + 17 * s + 1
            audio.append((rs.uniform(-0.3, 0.3, n) * (1 + s)).astype(F32))
            program, is_drum = ((0, False), (0, True), (33 + t, False))[s]
            ns = NoteSequence()
            for _ in range(40):
                st = float(rs.uniform(0, sec - 0.6))
                ns.notes.append(Note(st, st + float(rs.uniform(0.05, 0.5)), int(rs.randint(36, 84)), 90, program, is_drum, 0))
            ns.total_time = max(n_.end_time for n_ in ns.notes)
            notes.append(ns)
            programs.append((program, is_drum))
        tracks.append(StemTrack("track%02d" % t, ["s%d" % s for s in range(len(seconds))], audio, notes, programs))
    return tracks


def write_tracks(root, tracks):
    """The tracks as a stem folder under `root` (16-bit WAV + MIDI per stem), with the project's own writers."""
    import os
    from contrib import audio_io, midi_io
    for tr in tracks:
        d = os.path.join(str(root), tr.name)
        os.makedirs(os.path.join(d, "stems"))
        os.makedirs(os.path.join(d, "MIDI"))
        for name, a, ns in zip(tr.stem_names, tr.audio, tr.notes):
            audio_io.write_wav(os.path.join(d, "stems", name + ".wav"), a)
            midi_io.note_sequence_to_midi_file(ns, os.path.join(d, "MIDI", name + ".mid"))
    return str(root)
