"""StemMixBatcher.build end to end, host labels against device labels, on one MI355X.

    python profiles/tools/device_labels_bench.py [--out profiles/r22_device_labels.txt] [--runs 5] [--rows 64]

A synthetic Slakh-sized track (8 stems x 800 notes x 240 s, one drum stem), a 64-row batch with fresh stem subsets in every
row and every run, `device_labels` off and on in the same process, alternated, `--runs` times each, for `pitch_shift` 0 and
12; wall time around `build` + a device synchronisation.  Then the label launch alone, by device events.  A report, not a
target: the host path is this tree's own, unchanged.
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "mr-mt3_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def slakh_sized_track(seconds=240.0, n_stems=8, n_notes=800, seed=0):
    from contrib.note_sequences import Note, NoteSequence
    from mrmt3.stems import StemTrack
    rs = np.random.RandomState(seed)
    audio, notes, programs = [], [], []
    for s in range(n_stems):
        program, drum = (0, True) if s == 1 else (8 * s, False)
        ns = NoteSequence()
        for _ in range(n_notes):
            st = float(rs.uniform(0, seconds - 1.0))
            ns.notes.append(Note(st, st + float(rs.uniform(0.05, 0.8)), int(rs.randint(36, 84)), 90, program, drum, 0))
        ns.total_time = max(n.end_time for n in ns.notes)
        audio.append((rs.uniform(-0.1, 0.1, int(seconds * 16000) - 13 * s)).astype(np.float32))
        notes.append(ns)
        programs.append((program, drum))
    return StemTrack("slakh_sized", ["s%d" % s for s in range(n_stems)], audio, notes, programs)


def main():
    import torch
    from mrmt3 import lib
    from mrmt3.batching import StemMixBatcher
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_device_labels.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    track = slakh_sized_track()
    lines = ["device labels against host labels: StemMixBatcher.build end to end, %d rows, 8 stems x 800 notes x 240 s, %s"
             % (args.rows, torch.cuda.get_device_name(0)),
             "pitch_shift  labels  median_ms  min_ms  max_ms  (of %d builds, fresh subsets every row and run)" % args.runs]
    geom = dict(num_rows_per_batch=args.rows, split_frame_length=400, out_bf16=True)
    for shift in (0, 12):
        bts = {on: StemMixBatcher(dev, rng=random.Random(17), pitch_shift=shift, device_labels=on, **geom) for on in (False, True)}
        for bt in bts.values():
            bt.pool(track)                                   # the upload is not part of a build's time
        took = {False: [], True: []}
        last = {}
        for run in range(args.runs):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[on] = bts[on].build(track)
                torch.cuda.synchronize()
                took[on].append(1e3 * (time.perf_counter() - t0))
            assert torch.equal(last[False][1], last[True][1]), "host and device targets differ"
        for on in (False, True):
            lines.append("%11d  %6s  %9.2f  %6.2f  %6.2f" % (shift, "device" if on else "host", statistics.median(took[on]),
                                                             min(took[on]), max(took[on])))
        lines.append("%11d  ratio host / device (medians): %.1f; rows rebuilt on the host: %d"
                     % (shift, statistics.median(took[False]) / statistics.median(took[True]), bts[True].host_label_rows))
        if shift == 12:                                      # the label launch alone, by device events
            bt, plan = bts[True], bts[True].plan(track)
            bt.device_targets(track, plan)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            per = []
            for _ in range(args.runs):
                n0 = lib.label_launches()
                e0.record()
                for _ in range(20):
                    bt.device_targets(track, plan)
                e1.record()
                torch.cuda.synchronize()
                per.append(1e3 * e0.elapsed_time(e1) / (lib.label_launches() - n0))
            lines.append("label launch + argument copy + status read-back (20 per figure, device events): median %.1f us, "
                         "min %.1f, max %.1f" % (statistics.median(per), min(per), max(per)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
