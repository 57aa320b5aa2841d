"""Times of the resampler on one MI355X: `mrmt3_resample_mix_fwd` + `mrmt3_logmel_fwd` for 64 rows x 32768
samples out of 8 sources at a shift of +3 semitones, next to `mrmt3_logmel_mix_fwd` (the unshifted launch) at the same
shape, the variants timed in turn RUNS times over (ITERS launches each, device events around them) so that drift of the
box hits all alike; the resampler alone with its staged (LDS) and its global reader; and the one-off resample of a
4-minute 44.1 kHz stem to 16 kHz.  First checks one row of the timed shape against the numpy restatement, bit for bit.

    python profiles/tools/resample_mix_bench.py"""
import os
import sys
from fractions import Fraction

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "mr-mt3_amd"), ROOT, os.path.join(ROOT, "tests")]
from contrib import spectrograms as sp                                   # noqa: E402
from mrmt3 import lib                                                     # noqa: E402
from mrmt3.resample import ONE, device_filter, out_length, ratio_step, resample, resample_filter   # noqa: E402

RUNS, ITERS, B, F, HOP, S = 5, 200, 64, 256, 128, 8
dev = torch.device("cuda:0")
lib.load()
tabs = sp.kernel_tables(sp.SpectrogramConfig(), dev)
n = F * HOP
step = ratio_step(2.0 ** (3 / 12.0))
L = ((B * n * step) >> 32) + 8192                                          # one stem: room for 64 disjoint stretched crops
pool = torch.rand(S * L, device=dev) * 2 - 1
rows = torch.arange(B, dtype=torch.int64, device=dev)
begin = (torch.arange(S, dtype=torch.int64, device=dev)[None, :] * L).expand(B, S).contiguous()
end = (begin + L).contiguous()
pos = ((begin + 64) << 32) + (rows[:, None] * n + 2 * rows[:, None] + 1) * step
steps = torch.full((B, S), step, dtype=torch.int64, device=dev)
gain = torch.full((B, S), 0.5, device=dev)
gain[:, 0] = 1.0
fidx = torch.zeros(B, S, dtype=torch.int32, device=dev)
filt = device_filter(step, dev)
valid = torch.full((B,), n, dtype=torch.int64, device=dev)
vf = torch.full((B,), F, dtype=torch.int32, device=dev)
start_mix = (pos >> 32).contiguous()


def shifted():
    return lib.logmel(lib.resample_mix(pool, pos, begin, end, steps, gain, fidx, n, filt, valid), tabs, valid_frames=vf,
                      out_bf16=True)


def resample_only():
    return lib.resample_mix(pool, pos, begin, end, steps, gain, fidx, n, filt, valid)


def unshifted():
    return lib.logmel_mix(pool, start_mix, end, gain, n, tabs, valid_frames=vf, out_bf16=True)


def with_knob(fn, value):
    def run():
        lib.set_knob("MRMT3_RESAMPLE_LDS", value)
        return fn()
    return run


# one row of the timed shape against the restatement
import _resample as rsm                                                    # noqa: E402
got = resample_only()[5].cpu().numpy()
c = lambda t: t[5:6].cpu().numpy()
want = rsm.resample_rows(pool.cpu().numpy(), c(pos), c(begin), c(end), c(steps), c(gain), c(fidx), n,
                         resample_filter(Fraction(step, ONE))[None])[0]
assert np.array_equal(got.view(np.int32), want.view(np.int32)), "the kernel differs from the restatement at the timed shape"
print("row 5 of %d x %d, %d sources, step %.6f, %d taps: equals the restatement bit for bit" % (B, n, S, step / ONE, filt.shape[2]))


def time_variants(variants, iters):
    for _, fn in variants:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(RUNS):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / iters)
    for name, _ in variants:
        v = sorted(times[name])
        print("%-46s median %9.1f us   min %9.1f   max %9.1f" % (name, v[len(v) // 2], v[0], v[-1]))


print("us per call, %d runs x %d calls, variants in turn" % (RUNS, ITERS))
time_variants([("logmel_mix (unshifted launch, 8 sources)", unshifted),
               ("resample_mix + logmel (k = +3, 8 sources)", with_knob(shifted, 1)),
               ("resample_mix alone, staged reader", with_knob(resample_only, 1)),
               ("resample_mix alone, global reader", with_knob(resample_only, 0))], ITERS)
lib.reset_knobs()

# the one-off of an upload: a 4-minute stem at 44.1 kHz -> 16 kHz
x = torch.rand(4 * 60 * 44100, device=dev) * 2 - 1
y = resample(x, 44100, 16000)
assert y.numel() == out_length(x.numel(), ratio_step(Fraction(44100, 16000)))
print("4-minute 44.1 kHz stem: %d -> %d samples, %d taps" % (x.numel(), y.numel(), device_filter(ratio_step(Fraction(44100, 16000)), dev).shape[2]))
time_variants([("resample 4 min 44.1 kHz -> 16 kHz", lambda: resample(x, 44100, 16000))], 20)
