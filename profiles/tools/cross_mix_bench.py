"""The label launch for rows of virtual tracks against the single-track launch, and StemMixBatcher.build with the
cross-track options off and on, on one MI355X.

    python profiles/tools/cross_mix_bench.py [--out profiles/r28_cross_mix.txt] [--runs 5] [--rows 64]

Synthetic Slakh-sized tracks (8 stems x 800 notes x 240 s, one drum stem; partners on other programs).  The label launch
for `--rows` rows plus as many previous windows, by device events, 20 launches per figure: mrmt3_label_rows_fwd, the new
entry with one part (the same rows), the new entry with 3 parts — each in turn with the old entry on the same rows, in the
same process, `--runs` times over.  Then `build` end to end (wall time around build + a device synchronisation) with the
options off and with two partners and per-row shifts.  A report, not a target.
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "mr-mt3_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def partner_track(k):
    """`slakh_sized_track` on programs no other track of the run plays (and no drum stem)."""
    import dataclasses
    from device_labels_bench import slakh_sized_track
    tr = slakh_sized_track(seed=k)
    programs = [(8 * s + k, False) for s in range(len(tr.audio))]
    for ns, (program, drum) in zip(tr.notes, programs):
        ns.notes = [dataclasses.replace(n, program=program, is_drum=drum) for n in ns.notes]
    return dataclasses.replace(tr, name="partner%d" % k, programs=programs)


def timed(fn, runs, per=20):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(runs):
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / per)
    return out


def main():
    import torch
    from device_labels_bench import slakh_sized_track
    from mrmt3 import lib
    from mrmt3.batching import StemMixBatcher
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_cross_mix.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tracks = [slakh_sized_track()] + [partner_track(k) for k in (1, 2)]
    geom = dict(num_rows_per_batch=args.rows, split_frame_length=400, out_bf16=True, device_labels=True, with_prev=True)
    lines = ["cross-track rows: the label launch and StemMixBatcher.build, %d rows + %d previous windows, tracks of 8 stems x "
             "800 notes x 240 s, %s" % (args.rows, args.rows, torch.cuda.get_device_name(0))]

    # ---- the label launch alone: the same rows through both entries ----
    bt = StemMixBatcher(dev, rng=random.Random(17), cross_track=True, cross_prob=1.0, per_row_shift=True, pitch_shift=4, **geom)
    plans = {1: bt.plan_cross(tracks[0]), 3: bt.plan_cross(tracks[0], tracks[1:])}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64 else a)).to(dev)
    calls = {}
    for parts, plan in plans.items():
        _, _, times, meta, first, count = bt._resident(plan)
        arrays = [up(a) for a in bt.cross_label_arrays(plan, first, count)]
        calls["new entry, %d part%s" % (parts, "s" if parts > 1 else "")] = (
            lambda a=arrays, t=times, m=meta: lib.label_rows_parts(t, m, *a, bt._codec, bt.event_length))
        if parts == 1:                       # the same rows as mrmt3_label_rows_fwd takes them
            nf, nc, kp, dl, sc, sh, f0, n, total = arrays
            t1, m1 = times[first[0]:first[0] + count[0]], meta[first[0]:first[0] + count[0]]
            flat = [x.reshape(-1).contiguous() for x in (kp, sc, sh)]
            old = lambda: lib.label_rows(t1, m1, 8, flat[0], f0, n, total, flat[1], flat[2], bt._codec, bt.event_length)
            a, b = old(), calls["new entry, 1 part"]()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the two entries differ on one-part rows"
    lines.append("entry                 median_us  min_us  max_us   old entry in the same turn: median_us  min_us  max_us  "
                 "(20 launches per figure, %d figures, device events)" % args.runs)
    for name, fn in [("old entry", old)] + list(calls.items()):
        mine, ref = [], []
        for _ in range(args.runs):
            ref += timed(old, 1)
            mine += timed(fn, 1)
        lines.append("%-20s  %9.1f  %6.1f  %6.1f   %37.1f  %6.1f  %6.1f" % (
            name, statistics.median(mine), min(mine), max(mine), statistics.median(ref), min(ref), max(ref)))
    status = calls["new entry, 3 parts"]()[1]
    lines.append("rows of the 3-part launch with status != 0: %d of %d" % (int((status != 0).sum()), status.numel()))

    # ---- build end to end ----
    lines.append("build                      median_ms  min_ms  max_ms  (of %d builds, fresh plans, wall time + synchronize)" % args.runs)
    off = StemMixBatcher(dev, rng=random.Random(3), **geom)
    on = StemMixBatcher(dev, rng=random.Random(3), cross_track=True, per_row_shift=True, pitch_shift=4, **geom)
    for t in tracks:
        on.pool(t)
    off.pool(tracks[0])
    took = {"options off": [], "cross=2, per_row_shift": []}
    for run in range(args.runs + 1):
        for name, fn in (("options off", lambda: off.build(tracks[0])),
                         ("cross=2, per_row_shift", lambda: on.build(tracks[0], partners=tracks[1:]))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if run:                          # (the first build of each warms the filter tables and the allocator)
                took[name].append(1e3 * (time.perf_counter() - t0))
    for name, v in took.items():
        lines.append("%-25s  %9.2f  %6.2f  %6.2f" % (name, statistics.median(v), min(v), max(v)))
    lines.append("rows rebuilt on the host with the options on: %d" % on.host_label_rows)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
