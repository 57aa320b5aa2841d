"""Tokens -> notes, the host stage against the device stage, on one MI355X.

    python profiles/tools/device_notes_bench.py [--out profiles/r23_device_notes.txt] [--runs 20]

Decoded ids of 1, 8, 64 and 256 segments of one recording, resident on the device as the decoder leaves them, at two token
densities (about 233 and 895 tokens a segment: `tie`, then shift, `program, velocity, pitch` groups, ons and offs).  Timed on
the same ids in the same process, alternated, after a warm-up, the median of `--runs`:
  host    `postprocess_batch` + `InferenceHandler._to_event`      (the copy of the ids to the host included)
  device  `mrmt3.notes.decode_notes` + `NoteArrays.to_note_sequence`   (the launch, the compact copy back, the Note objects)
and beside them the launch alone by device events and `to_note_sequence` alone.  Both give the same note sequence, which
is checked.  A report, not a target.
"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "mr-mt3_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def segment_ids(n_seg, events, codec, ld=1024, seed=0):
    """[n_seg, ld] int64 model ids: per segment the tie section of what sounds, `tie`, then `events` groups of (shift,)
    program, velocity, pitch at sorted random steps — an off for a sounding note every other group."""
    from contrib import vocabularies
    sp = vocabularies.NUM_SPECIAL_TOKENS
    lo = {t: codec.event_type_range(t)[0] + sp for t in ("shift", "pitch", "velocity", "tie", "program")}
    rs = np.random.RandomState(seed)
    ids = np.zeros((n_seg, ld), np.int64)
    sounding = []
    for s in range(n_seg):
        row = []
        for program, pitch in sounding[:40]:
            row += [lo["program"] + program, lo["pitch"] + pitch]
        sounding = sounding[:40]
        row.append(lo["tie"])
        cur = 0
        for k, step in enumerate(sorted(rs.randint(0, 205, size=events).tolist())):
            if step > cur:
                row.append(lo["shift"] + step)
                cur = step
            if k % 2 and sounding:
                program, pitch = sounding.pop(rs.randint(len(sounding)))
                row += [lo["program"] + program, lo["velocity"], lo["pitch"] + pitch]
            else:
                program, pitch = int(rs.randint(8)) * 8, int(rs.randint(36, 96))
                row += [lo["program"] + program, lo["velocity"] + 1, lo["pitch"] + pitch]
                if (program, pitch) not in sounding:
                    sounding.append((program, pitch))
        row = row[:ld - 2] + [1]
        ids[s, 1:1 + len(row)] = row
    return ids


def median_ms(fn, runs, warm=3):
    import torch
    took = []
    for i in range(warm + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            took.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(took), min(took), max(took)


def main():
    import torch
    import inference
    from contrib import vocabularies
    from mrmt3 import lib, notes
    from mrmt3.grammar import EventGrammar
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_device_notes.txt"))
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    stub = types.SimpleNamespace(codec=codec)
    lines = ["tokens -> notes, host stage against device stage, %s; ms, median (min .. max) of %d runs after 3 warm-up runs"
             % (torch.cuda.get_device_name(0), args.runs),
             "segments  tokens   notes  host_ms                 device_ms              host/device  kernel_ms  to_note_sequence_ms  share"]
    for events in (60, 255):
        for n_seg in (1, 8, 64, 256):
            ids_np = segment_ids(n_seg, events, codec)
            ft = np.arange(n_seg * 256).reshape(n_seg, 256) / 125.0
            ids = torch.from_numpy(ids_np).to(dev)
            tokens = int((np.cumsum(ids_np[:, 1:] == 1, axis=1) == 0).sum())

            def host():
                return inference.InferenceHandler._to_event(stub, [inference.postprocess_batch(ids)], [ft])

            def device():
                return notes.decode_notes(ids, ft, codec)[0].to_note_sequence()

            a, b = host(), device()
            assert a.notes == b.notes and a.total_time == b.total_time and \
                [n.instrument for n in a.notes] == [n.instrument for n in b.notes], "host and device notes differ"
            h, d = median_ms(host, args.runs), median_ms(device, args.runs)
            arrays = notes.decode_notes(ids, ft, codec)[0]
            t = median_ms(arrays.to_note_sequence, args.runs)
            # the launch alone, by device events, on prepared arguments
            seg_first, start, limit, _ = notes.segment_times(ft, codec)
            up = lambda x: torch.from_numpy(x).to(dev)
            g = EventGrammar.from_codec(codec)
            kargs = (g, ids, up(seg_first), up(start), up(limit), up(notes.velocity_table(codec)), 100)
            per = []
            for i in range(3 + args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = lib.notes_decode(*kargs)
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    per.append(e0.elapsed_time(e1))
            assert int(out["status"][0]) == 0
            k = statistics.median(per)
            lines.append("%8d  %6d  %6d  %6.2f (%6.2f .. %6.2f)  %6.2f (%5.2f .. %6.2f)  %11.1f  %9.3f  %19.2f  %4.0f %%"
                         % (n_seg, tokens, len(a.notes), h[0], h[1], h[2], d[0], d[1], d[2], h[0] / d[0], k, t[0],
                            100 * t[0] / d[0]))
    lines.append("host/device: ratio of the medians; kernel_ms: the launch of mrmt3_notes_decode_fwd alone (device events, the "
                 "output tensors' allocation included); share: to_note_sequence (Python Note objects) of the device path")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
