"""Note-level scores, the host scorer against the device scorer, on one MI355X.

    python profiles/tools/note_match_time.py [--out profiles/r24_note_match.txt] [--runs 10] [--host-seconds 100]

Synthetic material: dense multi-program notes on the 10 ms grid (100 notes a second, eight programs in four General-MIDI
families and drums), the estimate a copy with a tenth of the notes dropped, a tenth added and onsets moved by up to 40 ms.
Sizes 2000, 6000 and 20 000 notes a side, 1 and 16 recordings.  Timed in one process after a warm-up, median and range:
  host    `evaluate.compute_transcription_metrics` + `evaluate.mt3_program_aware_note_scores` at the three granularities,
          on MidiData already in memory (what `evaluate_main` computes per pair)
  device  `mrmt3.scoring.score_tables` on tables already on the device (problem lists, ONE launch, the read-back), and the
          launch alone by device events
The host is timed on ONE recording (16 recordings are a sequential loop over pairs: 16 times that).  A host repetition that
would not fit `--host-seconds` in `--runs` repetitions is repeated as often as fits, at least once; a size whose dense
matrices would not fit the box's free memory is not run, and the report says so.
Also: the longest run and the window lengths the matcher met, and `train.validate_notes` per validation track beside the
`val_loss` pass over the same tracks.  A report, not a target.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "mr-mt3_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

PROGRAMS = [(0, False), (1, False), (24, False), (25, False), (33, False), (40, False), (48, False), (56, False), (0, True)]


def material(n, seed):
    """(reference MidiData, estimated MidiData) of about n notes each."""
    from contrib import midi_io
    rng = np.random.default_rng(seed)
    seconds = n / 100.0
    ref = [[] for _ in PROGRAMS]
    for _ in range(n):
        start = float(rng.integers(0, int(seconds * 100))) * 0.01
        ref[int(rng.integers(0, len(PROGRAMS)))].append((start, start + float(rng.integers(2, 60)) * 0.01,
                                                         int(rng.integers(30, 100))))
    est = [[] for _ in PROGRAMS]
    for g, notes in enumerate(ref):
        for s, e, p in notes:
            if rng.random() < 0.1:
                continue
            s2 = max(0.0, s + float(rng.integers(-4, 5)) * 0.01)
            est[g].append((s2, s2 + max(0.01, e - s + float(rng.integers(-5, 6)) * 0.01), p))
        for _ in range(len(notes) // 10):
            s = float(rng.integers(0, int(seconds * 100))) * 0.01
            est[g].append((s, s + 0.1, int(rng.integers(30, 100))))
    mk = lambda groups: midi_io.MidiData([midi_io.MidiInstrument(pr, dr, [midi_io.MidiNote(s, e, p, 90) for s, e, p in notes])
                                          for (pr, dr), notes in zip(PROGRAMS, groups)], 220, seconds)
    return mk(ref), mk(est)


def host_scores(ref, est):
    import evaluate
    out = dict(evaluate.compute_transcription_metrics(ref, est))
    for g in ("flat", "full", "midi_class"):
        out.update(evaluate.mt3_program_aware_note_scores(ref, est, g))
    return out


def spread(times):
    return "%9.2f ms  (%.2f .. %.2f, n=%d)" % (1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times), len(times))


def run_lengths(problems, ref, est):
    """(longest run, largest window, mean window) over every problem, from the host restatement's windows."""
    from mrmt3 import scoring
    ref_t, est_t = ref.times.cpu().numpy(), est.times.cpu().numpy()
    ref_idx, est_idx = problems.ref_idx.cpu().numpy(), problems.est_idx.cpu().numpy()
    ref_first, est_first = problems.ref_first.cpu().numpy(), problems.est_first.cpu().numpy()
    longest, widest, total, count = 0, 0, 0, 0
    for p in range(len(problems.family)):
        r_on = ref_t[ref_idx[ref_first[p]:ref_first[p + 1]], 0]
        e_on = est_t[est_idx[est_first[p]:est_first[p + 1]], 0]
        if not len(r_on) or not len(e_on):
            continue
        lo = np.searchsorted(r_on, e_on - scoring.ONSET_TOLERANCE - 5e-7, "left")
        hi = np.searchsorted(r_on, e_on + scoring.ONSET_TOLERANCE + 5e-7, "right")
        starts = np.flatnonzero(np.concatenate([[True], lo[1:] >= hi[:-1]]))
        longest = max(longest, int(np.diff(np.concatenate([starts, [len(e_on)]])).max()))
        widest, total, count = max(widest, int((hi - lo).max())), total + int((hi - lo).sum()), count + len(e_on)
    return longest, widest, total / max(count, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_note_match.txt"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-seconds", type=float, default=100.0)
    ap.add_argument("--sizes", default="2000,6000,20000")
    a = ap.parse_args()
    import torch
    from mrmt3 import lib, scoring
    from mrmt3.notes import DeviceNotes
    dev = torch.device("cuda:0")
    lines = ["note-level scores: host scorer vs mrmt3.scoring.score_tables (DESIGN 4n); %s, %d repetitions after a warm-up"
             % (torch.cuda.get_device_name(0), a.runs), ""]
    say = lambda s: (lines.append(s), print(s, flush=True))
    free = int(next(l for l in open("/proc/meminfo") if l.startswith("MemAvailable")).split()[1]) * 1024
    for n in (int(v) for v in a.sizes.split(",")):
        pairs = [material(n, 100 + r) for r in range(16)]
        tabs = [[scoring.table_from_midi(m) for m in side] for side in zip(*pairs)]
        sizes = "%d / %d notes" % (len(tabs[0][0].meta), len(tabs[1][0].meta))
        # ---- host, one recording
        need = 6 * 8 * len(tabs[0][0].meta) * len(tabs[1][0].meta)      # onset, cents (three temporaries), offsets: f64 n x m
        host = None
        if need > free:
            say("%6d notes  host    not run: its dense matrices need about %.1f GB, the box has %.1f GB free"
                % (n, need / 1e9, free / 1e9))
        else:
            t0 = time.perf_counter()
            host = host_scores(*pairs[0])
            first = time.perf_counter() - t0
            reps = max(1, min(a.runs, int(a.host_seconds / max(first, 1e-3))))
            times = [first] if reps == 1 else []
            for _ in range(0 if reps == 1 else reps):
                t0 = time.perf_counter()
                host_scores(*pairs[0])
                times.append(time.perf_counter() - t0)
            say("%6d notes  host    1 recording (%s)   %s%s" % (n, sizes, spread(times),
                                                                "   [no warm-up: the only repetition]" if reps == 1 else ""))
        for R in (1, 16):
            ref = DeviceNotes.from_arrays(tabs[0][:R], dev)
            est = DeviceNotes.from_arrays(tabs[1][:R], dev)
            got = scoring.score_tables(ref, est)                       # warm-up; and the same numbers as the host's
            if host is not None:
                assert all(got[0][k] == v for k, v in host.items() if "overlap" not in k and k != "F1 by program")
            times = []
            for _ in range(a.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                scoring.score_tables(ref, est)
                times.append(time.perf_counter() - t0)
            problems = scoring.build_problems(ref, est)
            lo, hi = (torch.from_numpy(t).to(dev) for t in scoring.pitch_tables())
            kernel = []
            for _ in range(a.runs + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                lib.note_match(ref.times, ref.meta, est.times, est.meta, problems.ref_idx, problems.ref_first, problems.est_idx,
                               problems.est_first, problems.prob_flags, lo, hi)
                e1.record()
                torch.cuda.synchronize()
                kernel.append(e0.elapsed_time(e1) * 1e-3)
            longest, widest, mean = run_lengths(problems, ref, est)
            say("%6d notes  device  %2d recording%s, %3d problems   %s" % (n, R, " " if R == 1 else "s", len(problems.family),
                                                                          spread(times)))
            say("%6d notes  kernel  %2d recording%s                 %s   longest run %d entries, windows mean %.1f max %d"
                % (n, R, " " if R == 1 else "s", spread(kernel[1:]), longest, mean, widest))
        say("")
    # ---- validate_notes beside the val_loss pass
    import _stem_mix as sm
    import train
    from mrmt3.batching import StemMixBatcher
    from mrmt3.trainer import Trainer
    from test_train_infer_gpu import _model
    tracks = sm.synthetic_tracks(2)
    model = _model("t5", dev)
    trainer = Trainer(model, lr=1e-3)
    loader = train.StemLoader(tracks, StemMixBatcher(dev, is_deterministic=True, mel_length=256, event_length=1024,
                                                     num_rows_per_batch=2, split_frame_length=2000), 1, seed=5, shuffle=False)

    def val_loss():
        for b in loader:
            trainer.eval_loss(b[0], b[1]).sum().item()

    def val_notes():
        return train.validate_notes(model, tracks, dev)

    for name, fn in (("val_loss pass", val_loss), ("validate_notes", val_notes)):
        fn()
        times = []
        for _ in range(max(3, a.runs // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / len(tracks))
        say("%-15s per validation track (2 synthetic tracks of about 5 s, small T5, untrained: every segment decodes its "
            "full 1024 tokens)   %s" % (name, spread(times)))
    trainer.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
