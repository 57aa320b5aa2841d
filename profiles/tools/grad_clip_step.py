"""Cost of gradient clipping in the captured training step (Trainer(gradient_clip_val=...), mrmt3_grad_norm +
mrmt3_adamw_step with stat_dev): the 64-segment MT3Net step of bench.py (bf16, raw audio in, dropout on, graph replay), timed
with the feature off and on in ONE process, alternating blocks of steps, wall clock around each block with a device
synchronise; then the norm kernels alone on the model's G (device events), cache-warm and behind a 1 GiB flush.
    python3 profiles/tools/grad_clip_step.py [mode = ab|off|clip] [rounds = 6] [steps per block = 20]
`off` / `clip`: one trainer, rounds x steps replayed steps and nothing else — the form to put under a kernel trace."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "mr-mt3_amd"), ROOT):
    sys.path.insert(0, p)
import torch

from mrmt3 import lib
from mrmt3.synthetic import T5_SMALL, synth_audio, synth_labels
from mrmt3.trainer import Trainer

MODE = sys.argv[1] if len(sys.argv) > 1 else "ab"
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 6
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
B, N_SAMPLES = 64, 256 * 128
dev = torch.device("cuda:0")


def trainer(clip):
    from models.t5 import T5ForConditionalGeneration
    m = T5ForConditionalGeneration(T5_SMALL).load_golden().to(dev)
    from utils import cosine_warmup_lambda
    lam = cosine_warmup_lambda(64500, 1289 * 800, min_lr=1e-4)       # bench.py's schedule: the same host work per step
    return Trainer(m, lr=2e-4, lr_lambda=lam, **({"gradient_clip_val": 1.0} if clip else {}))


def block(tr, audio, labels, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.train_step(audio, labels, None, audio=True)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    audio = torch.from_numpy(synth_audio(B, N_SAMPLES, seed=365)).to(dev)
    labels = torch.from_numpy(synth_labels(B, seed=365)).to(dev)
    names = {"ab": ["off", "clip"], "off": ["off"], "clip": ["clip"]}[MODE]
    trs = {k: trainer(k == "clip") for k in names}
    for tr in trs.values():
        while tr.use_graph and not tr.graph_captured:
            tr.train_step(audio, labels, None, audio=True)
        block(tr, audio, labels, 3)
    ms = {k: [] for k in names}
    for _ in range(ROUNDS):
        for k in names:
            ms[k].append(block(trs[k], audio, labels, STEPS))
    out = {"segments": B, "rounds": ROUNDS, "steps_per_block": STEPS,
           "ms_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()},
           "graph": {k: bool(t.graph_captured) for k, t in trs.items()}}
    if MODE == "ab":
        out["clip_minus_off_ms"] = out["ms_per_step"]["clip"]["median"] - out["ms_per_step"]["off"]["median"]
        tr = trs["clip"]
        out["grad_norm"], out["coef"] = float(tr.last_grad_norm.item()), float(tr._clip_stat[1].item())
        g = tr.flat.G
        ws, stat = lib.grad_norm_workspace(dev), torch.zeros(4, device=dev)
        skipped = torch.zeros(1, device=dev, dtype=torch.int32)
        flush = torch.empty(1 << 28, device=dev)             # 1 GiB: four times the Infinity Cache
        for name, cold in (("warm", False), ("flushed", True)):
            us = []
            for _ in range(20):
                if cold:
                    flush.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                lib.grad_norm(g, 1.0, 1.0, False, ws, stat, skipped)
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1))
            med = statistics.median(us)
            out["norm_kernels_us_" + name] = {"median": med, "min": min(us), "gbytes_per_s": g.numel() * 4 / med / 1e3}
        out["g_bytes"] = g.numel() * 4
    for tr in trs.values():
        tr.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
