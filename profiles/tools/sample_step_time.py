"""Time per token step of the KV-cached decoder (bf16, EOS disabled) with the greedy tail and with the sampled tail
(DESIGN §4f), measured with device events over N replays of the captured step after the decode has reached position t:
   python3 profiles/tools/sample_step_time.py [N] [t] [windows]            (default N = 64, t = 256, 5 windows)
One line per (batch, mode); the modes alternate and every figure is the median of the windows.  For the tail kernels' own times:
   rocprofv3 --kernel-trace --stats -- python3 profiles/tools/sample_step_time.py 64 64 1"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mr-mt3_amd"))
import torch  # noqa: E402
from mrmt3 import lib  # noqa: E402
from mrmt3.decode import Decoder  # noqa: E402
from mrmt3.synthetic import T5_SMALL, synth_mel  # noqa: E402
from models.t5 import T5ForConditionalGeneration  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T0 = int(sys.argv[2]) if len(sys.argv) > 2 else 256
WINDOWS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
MODES = {"greedy": None, "sample T=1": (1.0, 0, 1.0), "sample k=7": (1.0, 7, 1.0), "sample p=.9": (1.0, 0, 0.9),
         "sample T=.7 k=50 p=.9": (0.7, 50, 0.9)}
dev = torch.device("cuda:0")
m = T5ForConditionalGeneration(T5_SMALL, compute_dtype=torch.bfloat16).load_golden().to(dev).eval()
with torch.no_grad():
    m.flat.master("lm_head.weight")[1].zero_()          # no EOS: nothing finishes, every step does full work
m.engine.prepare(False)
d, Lc = m.cfg["d_model"], 256
l = lib.load()


def window_ms(dec, ckv, rows, mode):
    w = dec._weights()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dec.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(dec.stream):
        lib._check(l.mrmt3_decoder_begin(dec.h, C.byref(w), lib._p(ckv), rows, Lc, lib._p(dec.tokens), 0, 1, 0, lib._stream()),
                   "begin")
        if MODES[mode] is not None:
            T, k, p = MODES[mode]
            lib._check(l.mrmt3_decoder_set_sampling(dec.h, T, k, p, 11, lib._stream()), "set_sampling")
        lib._check(l.mrmt3_decoder_run(dec.h, T0, lib._stream()), "run")      # capture + warm-up up to position t
        e0.record()
        lib._check(l.mrmt3_decoder_run(dec.h, N, lib._stream()), "run")
        e1.record()
    torch.cuda.synchronize()
    assert dec.graph_captured
    return e0.elapsed_time(e1) / N


print(f"bf16 T5-small decoder, ms per token step over {N} replays from position {T0} (device events, median of {WINDOWS})")
for rows in (1, 8, 64):
    dec = Decoder(m, rows, 1024, Lc)
    mel = torch.from_numpy(synth_mel(rows, seed=3)).to(dev)
    with torch.no_grad():
        ckv = dec.cross_kv(m.engine.encode(mel).reshape(rows * Lc, d), rows, Lc)
    got = {k: [] for k in MODES}
    for rep in range(1 + WINDOWS):                            # the first round of windows warms every capture up
        for mode in MODES:
            ms = window_ms(dec, ckv, rows, mode)
            if rep:
                got[mode].append(ms)
    g = statistics.median(got["greedy"])
    for mode in MODES:
        v = statistics.median(got[mode])
        print(f"B={rows:2d}  {mode:24s} {v:.4f} ms/step  ({(v - g) * 1e3:+7.1f} us, {(v / g - 1) * 100:+5.1f} %)   "
              f"windows {' '.join(f'{x:.4f}' for x in got[mode])}", flush=True)
