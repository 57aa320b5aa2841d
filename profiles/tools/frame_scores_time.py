"""Frame scores, the host scorer against the device scorer, on one MI355X.

    python profiles/tools/frame_scores_time.py [--out profiles/r25_frame_scores.txt] [--runs 10]

The material of profiles/tools/note_match_time.py: dense multi-program notes on the 10 ms grid (100 notes a second), the
estimate a disturbed copy.  Sizes 2000, 6000 and 20 000 notes a side, 1 and 16 recordings.  Timed in one process after a
warm-up, median and range:
  host     `evaluate.host_frame_result` at "on" and the three granularities, on MidiData already in memory: the frame part of
           what `evaluate_main(frames=True)` computes per pair.  ONE recording (16 are a sequential loop: 16 times that)
  device   `mrmt3.scoring.score_tables(frames=True)` on tables already on the device (problem lists, the matcher, the frame
           kernel, ONE read-back), and `score_tables()` as it was: the difference is what the option costs
  kernel   `lib.note_frames` alone by device events, without and with the rolls written
A report, not a target.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "mr-mt3_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__)), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from note_match_time import material, spread  # noqa: E402


def host_frames(ref, est):
    import evaluate
    return evaluate.host_frame_result(ref, est, ("flat", "full", "midi_class"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_frame_scores.txt"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sizes", default="2000,6000,20000")
    a = ap.parse_args()
    import torch
    from mrmt3 import lib, scoring
    from mrmt3.notes import DeviceNotes
    dev = torch.device("cuda:0")
    lines = ["frame scores: evaluate.py's host scorer vs mrmt3.scoring.score_tables(frames=True) (DESIGN 4o); %s, %d repetitions "
             "after a warm-up" % (torch.cuda.get_device_name(0), a.runs), ""]
    say = lambda s: (lines.append(s), print(s, flush=True))

    def wall(fn):
        times = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return times

    for n in (int(v) for v in a.sizes.split(",")):
        pairs = [material(n, 100 + r) for r in range(16)]
        tabs = [[scoring.table_from_midi(m) for m in side] for side in zip(*pairs)]
        host = host_frames(*pairs[0])                                  # warm-up
        say("%6d notes  host    1 recording (%d / %d notes)      %s" % (n, len(tabs[0][0].meta), len(tabs[1][0].meta),
                                                                        spread(wall(lambda: host_frames(*pairs[0])))))
        for R in (1, 16):
            ref = DeviceNotes.from_arrays(tabs[0][:R], dev)
            est = DeviceNotes.from_arrays(tabs[1][:R], dev)
            got = scoring.score_tables(ref, est, frames=True)          # warm-up; and the same numbers as the host's
            assert all(got[0][k] == v for k, v in host.items()), (host, got[0])
            scoring.score_tables(ref, est)
            with_frames = wall(lambda: scoring.score_tables(ref, est, frames=True))
            without = wall(lambda: scoring.score_tables(ref, est))
            problems = scoring.build_problems(ref, est)
            n_frames = scoring.frames_for(problems.max_end)
            kernel = {False: [], True: []}
            for with_roll in (False, True):
                for _ in range(a.runs + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    lib.note_frames(ref.times, ref.meta, est.times, est.meta, problems.ref_idx, problems.ref_first,
                                    problems.est_idx, problems.est_first, scoring.FRAMES_PER_SECOND, n_frames, with_roll=with_roll)
                    e1.record()
                    torch.cuda.synchronize()
                    kernel[with_roll].append(e0.elapsed_time(e1) * 1e-3)
            rec = "%2d recording%s" % (R, " " if R == 1 else "s")
            say("%6d notes  device  %s, %3d problems, frames on    %s" % (n, rec, len(problems.family), spread(with_frames)))
            say("%6d notes  device  %s, %3d problems, frames off   %s   added by the option: %.2f ms"
                % (n, rec, len(problems.family), spread(without),
                   1e3 * (statistics.median(with_frames) - statistics.median(without))))
            say("%6d notes  kernel  %s, %d frames, %d tiles          %s" % (n, rec, n_frames, -(-n_frames // 2048),
                                                                           spread(kernel[False][1:])))
            say("%6d notes  kernel  %s, with the rolls (%.1f MB)       %s"
                % (n, rec, len(problems.family) * 2 * 128 * -(-n_frames // 32) * 4 / 1e6, spread(kernel[True][1:])))
        say("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
