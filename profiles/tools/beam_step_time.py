"""Time per token step of the KV-cached decoder (bf16, EOS disabled) for greedy, greedy with a ban (the 127 program ids
of an empty `valid_programs`) and beam search, measured with device events over N replays of the captured step after
the decode has reached position t:
   python3 profiles/tools/beam_step_time.py [N] [t ...]            (default N = 32, t = 256 900)
One line per (mode, groups, beams, t).  Greedy runs at the same row count as the beam case next to it (G x k rows).
For per-kernel times of the select and reorder kernels:
   rocprofv3 --kernel-trace --stats -- python3 profiles/tools/beam_step_time.py 32 900"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mr-mt3_amd"))
import torch  # noqa: E402
from mrmt3 import lib  # noqa: E402
from mrmt3.decode import Decoder  # noqa: E402
from mrmt3.synthetic import T5_SMALL, synth_mel  # noqa: E402
from models.t5 import T5ForConditionalGeneration  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
TS = [int(a) for a in sys.argv[2:]] or [256, 900]
BAN = list(range(1135, 1262))
dev = torch.device("cuda:0")
m = T5ForConditionalGeneration(T5_SMALL, compute_dtype=torch.bfloat16).load_golden().to(dev).eval()
with torch.no_grad():
    m.flat.master("lm_head.weight")[1].zero_()          # no EOS: nothing finishes, every step does full work
m.engine.prepare(False)
cfg, d, Lc = m.cfg, m.cfg["d_model"], 256
l = lib.load()
decs = {}


def step_ms(mode, G, k, t):
    rows = G * k
    key = rows
    if key not in decs:
        decs[key] = Decoder(m, rows, 1024, Lc)
    dec = decs[key]
    mel = torch.from_numpy(synth_mel(G, seed=3)).to(dev)
    with torch.no_grad():
        enc = m.engine.encode(mel).reshape(G * Lc, d)
        if mode == "beam":
            ckv = dec.cross_kv_beam(enc, G, k, Lc)
        else:
            ckv = dec.cross_kv(enc.view(G, Lc, d).repeat_interleave(k, 0).reshape(rows * Lc, d), rows, Lc)
    w = dec._weights()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dec.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(dec.stream):
        if mode == "beam":
            dec.begin_beam(ckv, G, k, Lc, 0.4, dec.ban_mask(BAN))
        else:
            lib._check(l.mrmt3_decoder_begin(dec.h, C.byref(w), lib._p(ckv), rows, Lc, lib._p(dec.tokens),
                                             0, 1, 0, lib._stream()), "begin")
            if mode == "ban":
                dec._ban = dec.ban_mask(BAN)
                lib._check(l.mrmt3_decoder_set_ban(dec.h, lib._p(dec._ban), lib._stream()), "set_ban")
        lib._check(l.mrmt3_decoder_run(dec.h, t, lib._stream()), "run")      # capture + warm-up up to position t
        e0.record()
        lib._check(l.mrmt3_decoder_run(dec.h, N, lib._stream()), "run")
        e1.record()
    torch.cuda.synchronize()
    assert dec.graph_captured
    return e0.elapsed_time(e1) / N


print(f"bf16 T5-small decoder, ms per token step over {N} replays (device events)")
for t in TS:
    for G, k in [(1, 1), (1, 2), (1, 4), (1, 8), (8, 1), (8, 2), (8, 4), (8, 8)]:
        g = step_ms("greedy", G, k, t)
        gb = step_ms("ban", G, k, t)
        line = f"t={t:4d} G={G} k={k} rows={G * k:2d}  greedy {g:.4f}  greedy+ban {gb:.4f} ({(gb / g - 1) * 100:+.1f} %)"
        if k > 1:
            b = step_ms("beam", G, k, t)
            line += f"  beam {b:.4f} ({b / g:.3f} x greedy)"
        print(line, flush=True)
