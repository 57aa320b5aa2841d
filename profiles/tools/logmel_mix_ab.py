"""Same-process A/B of the stem-mix log-mel launch: `mrmt3_logmel_mix_fwd` at n_src = 1, 4, 8, 16 against
`mrmt3_logmel_crops_fwd` of another build of the library (the parent commit's, built with `make OUT=...`) and of this
one, 64 rows x 256 frames, bf16 output.  Both libraries are loaded into one process and the variants are timed in turn,
RUNS times over (ITERS launches each, device events around them), so drift of the box hits all alike.  First checks that
n_src = 1 at gain 1 equals the other build's crops launch bit for bit at the size that is timed.

    python profiles/tools/logmel_mix_ab.py PARENT_LIBMRMT3_HIP_SO"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "mr-mt3_amd"), ROOT]
from contrib import spectrograms as sp   # noqa: E402
from mrmt3 import lib                    # noqa: E402

RUNS, ITERS, B, F, HOP = 5, 200, 64, 256, 128
dev = torch.device("cuda:0")
new = lib.load()
old = C.CDLL(os.path.abspath(sys.argv[1]))
old.mrmt3_version.restype = C.c_int
res, args = lib._SIGS["mrmt3_logmel_crops_fwd"]
old.mrmt3_logmel_crops_fwd.restype, old.mrmt3_logmel_crops_fwd.argtypes = res, args
print("parent library version", old.mrmt3_version(), "this library", new.mrmt3_version())

t = sp.kernel_tables(sp.SpectrogramConfig(), dev)
n = F * HOP
S = 16
L = B * n + 4096                                       # one stem: room for 64 disjoint crops
pool = (torch.rand(S * L, device=dev) * 2 - 1)
rows = torch.arange(B, dtype=torch.int64, device=dev)
start_all = (torch.arange(S, dtype=torch.int64, device=dev)[None, :] * L + rows[:, None] * n + 2 * rows[:, None] + 1).contiguous()
end_all = ((torch.arange(S, dtype=torch.int64, device=dev)[None, :] + 1) * L).expand(B, S).contiguous()
vf = torch.full((B,), F, dtype=torch.int32, device=dev)
out = torch.empty(B, F, 512, device=dev, dtype=torch.bfloat16)
p, st = lib._p, lib._stream()
seg = start_all[:, 0].contiguous()


def crops(so):
    rc = so.mrmt3_logmel_crops_fwd(p(pool), pool.numel(), p(seg), B, n, HOP, p(t["window"]), p(t["twiddle"]), p(t["fb_start"]),
                                   p(t["fb_cnt"]), p(t["fb_w"]), 512, t["max_taps"], p(vf), 1, 1, p(out), st)
    assert rc == 0


def mix(k):
    s, e = start_all[:, :k].contiguous(), end_all[:, :k].contiguous()
    g = torch.full((B, k), 0.5, device=dev)
    g[:, 0] = 1.0

    def run():
        rc = new.mrmt3_logmel_mix_fwd(p(pool), pool.numel(), p(s), p(e), p(g), k, B, n, HOP, p(t["window"]), p(t["twiddle"]),
                                      p(t["fb_start"]), p(t["fb_cnt"]), p(t["fb_w"]), 512, t["max_taps"], p(vf), 1, 1, p(out), st)
        assert rc == 0
    return run


variants = [("crops parent", lambda: crops(old)), ("crops this", lambda: crops(new))] + [("mix n_src=%d" % k, mix(k)) for k in (1, 4, 8, 16)]
# n_src = 1 at gain 1 must be the crops launch bit for bit, at the size that is timed
crops(old)
ref = out.clone()
variants[2][1]()
torch.cuda.synchronize()
assert torch.equal(ref, out), "mix n_src=1 differs from the parent's crops launch"
print("mix n_src=1 == parent crops, bit for bit, at 64 x 256 frames")
for _, fn in variants:
    for _ in range(20):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in variants}
for r in range(RUNS):
    for name, fn in variants:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1000.0 / ITERS)
print("us per launch (%d launches per run, enqueue included), runs interleaved: %s" % (ITERS, " ".join("run%d" % i for i in range(RUNS))))
for name, _ in variants:
    v = times[name]
    print("%-14s %s   median %.1f  min %.1f  max %.1f" % (name, " ".join("%7.1f" % x for x in v), float(np.median(v)), min(v), max(v)))
print(lib.dispatch_counts())
