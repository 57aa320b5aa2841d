"""Same-process A/B of the training step with parameter groups: all-trainable against encoder frozen, against
only the memory modules trainable, and against all-trainable with EMA weights, graph replay on, dropout on, the benchmark's
synthetic batches.  Every trainer is built and captured first; then the configurations are timed in turn, `--rounds` times
over (`--steps` replays each, one device synchronise around them), so drift of the box hits all alike.

    python profiles/tools/param_groups_ab.py [--rounds 5] [--steps 30] [--out FILE]

Prints one line per configuration: the median of its rounds and their spread, in ms per step."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "mr-mt3_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

MEM_ONLY = ["encoder.*", "decoder.*", "decoder_embed_tokens.weight", "lm_head.weight", "proj.weight"]
CONFIGS = [  # name, variant, segments, trainer options
    ("t5 12 all", "t5", 12, {}),
    ("t5 12 ema", "t5", 12, dict(ema_decay=0.999)),
    ("t5 12 encoder frozen", "t5", 12, dict(frozen=["encoder.*"])),
    ("t5 12 encoder frozen + no-decay norms + ema", "t5", 12,
     dict(frozen=["encoder.*"], no_decay=["*layer_norm.weight"], ema_decay=0.999)),
    ("with_prev 12 all", "segmem_v2_with_prev", 12, {}),
    ("with_prev 12 memory modules only", "segmem_v2_with_prev", 12, dict(frozen=MEM_ONLY)),
    ("t5 64 all", "t5", 64, {}),
    ("t5 64 ema", "t5", 64, dict(ema_decay=0.999)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bench import build_model
    from mrmt3.synthetic import synth_audio, synth_labels
    from mrmt3.trainer import Trainer
    dev = torch.device("cuda", 0)
    runs = []
    for name, variant, B, kw in CONFIGS:
        tr = Trainer(build_model(variant, dev), lr=2e-4, **kw)
        audio = torch.from_numpy(synth_audio(B, 32768, seed=365)).to(dev)
        labels = torch.from_numpy(synth_labels(B, seed=365)).to(dev)
        prev = torch.from_numpy(synth_labels(B, seed=1365)).to(dev) if variant == "segmem_v2_with_prev" else None
        step = (lambda tr=tr, audio=audio, labels=labels, prev=prev:
                tr.train_step(audio, labels, None if prev is None else prev.clone(), audio=True))
        while not tr.graph_captured:
            step()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        n_train = tr.flat.opt_ranges.n_trainable if tr.groups_on else tr.flat.numel
        runs.append(dict(name=name, step=step, tr=tr, ms=[], trainable=n_train))
        print("captured: %s (%d of %d elements trainable)" % (name, n_train, tr.flat.numel), flush=True)
    for _ in range(a.rounds):
        for r in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = r["step"]()
            torch.cuda.synchronize()
            r["ms"].append(1e3 * (time.perf_counter() - t0) / a.steps)
            r["loss"] = float(loss.item())
    rows = []
    for r in runs:
        row = dict(name=r["name"], trainable=r["trainable"], ms_median=statistics.median(r["ms"]), ms_min=min(r["ms"]),
                   ms_max=max(r["ms"]), rounds=r["ms"], final_loss=r["loss"])
        rows.append(row)
        print("%-48s %7.3f ms per step (rounds %.3f .. %.3f), loss %.4f"
              % (row["name"], row["ms_median"], row["ms_min"], row["ms_max"], row["final_loss"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    for r in runs:
        r["tr"].close()


if __name__ == "__main__":
    main()
