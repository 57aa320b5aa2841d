"""Time per token step of the KV-cached decoder (bf16) unconstrained and under the event grammar, measured with
device events over N replays of the captured step after the decode has reached position t:
   python3 profiles/tools/grammar_step_time.py [N] [t] [windows]            (default N = 64, t = 64, 5 windows)
Greedy at 1, 8 and 64 rows and beam search with k = 4 (8 groups); the two modes alternate on one decoder, in the same
process, and every figure is the median of the windows.  The lm_head row of EOS is zeroed so that rows keep going; the last
column says how many rows had emitted EOS by the end of the window all the same (a finished row skips the grammar kernel)."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mr-mt3_amd"))
import torch  # noqa: E402
from contrib import vocabularies  # noqa: E402
from mrmt3 import lib  # noqa: E402
from mrmt3.decode import Decoder  # noqa: E402
from mrmt3.grammar import EventGrammar  # noqa: E402
from mrmt3.synthetic import T5_SMALL, synth_mel  # noqa: E402
from models.t5 import T5ForConditionalGeneration  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
T0 = int(sys.argv[2]) if len(sys.argv) > 2 else 64
WINDOWS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda:0")
m = T5ForConditionalGeneration(T5_SMALL, compute_dtype=torch.bfloat16).load_golden().to(dev).eval()
with torch.no_grad():
    m.flat.master("lm_head.weight")[1].zero_()
m.engine.prepare(False)
d, Lc = m.cfg["d_model"], 256
l = lib.load()
G = EventGrammar.from_codec(vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))).c_struct()


def window(dec, ckv, rows, k, constrained):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dec.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(dec.stream):
        if k:
            dec.begin_beam(ckv, rows // k, k, Lc, 0.4, None)
        else:
            w = dec._weights()
            lib._check(l.mrmt3_decoder_begin(dec.h, C.byref(w), lib._p(ckv), rows, Lc, lib._p(dec.tokens), 0, 1, 0, lib._stream()),
                       "begin")
        if constrained:
            lib._check(l.mrmt3_decoder_set_grammar(dec.h, C.byref(G), None, lib._stream()), "set_grammar")
        lib._check(l.mrmt3_decoder_run(dec.h, T0, lib._stream()), "run")      # capture + warm-up up to position t
        e0.record()
        lib._check(l.mrmt3_decoder_run(dec.h, N, lib._stream()), "run")
        e1.record()
    torch.cuda.synchronize()
    assert dec.graph_captured
    finished = int((dec.tokens[:rows, 1:T0 + N + 1] == 1).any(1).sum())
    return e0.elapsed_time(e1) / N, finished


print(f"bf16 T5-small decoder, ms per token step over {N} replays from position {T0} (device events, median of {WINDOWS})")
for rows, k in ((1, 0), (8, 0), (64, 0), (32, 4)):
    dec = Decoder(m, rows, 1024, Lc)
    segs = rows // k if k else rows
    mel = torch.from_numpy(synth_mel(segs, seed=3)).to(dev)
    with torch.no_grad():
        enc = m.engine.encode(mel).reshape(segs * Lc, d)
        ckv = dec.cross_kv_beam(enc, segs, k, Lc) if k else dec.cross_kv(enc, rows, Lc)
    got = {False: [], True: []}
    fin = {}
    for rep in range(1 + WINDOWS):                            # the first round of windows warms both captures up
        for c in (False, True):
            ms, fin[c] = window(dec, ckv, rows, k, c)
            if rep:
                got[c].append(ms)
    a, b = statistics.median(got[False]), statistics.median(got[True])
    name = f"beam k={k} x {segs}" if k else f"greedy B={rows}"
    print(f"{name:16s} unconstrained {a:.4f} ms/step = {rows / (k or 1) / a * 1e3:9.0f} tok/s   constrained {b:.4f} ms/step = "
          f"{rows / (k or 1) / b * 1e3:9.0f} tok/s   ({(b - a) * 1e3:+6.1f} us, {(b / a - 1) * 100:+5.1f} %)   rows with EOS "
          f"{fin[False]} / {fin[True]}   windows {' '.join(f'{x:.4f}' for x in got[False])} | "
          f"{' '.join(f'{x:.4f}' for x in got[True])}", flush=True)
