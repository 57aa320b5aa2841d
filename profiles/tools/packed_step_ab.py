"""Dense against packed decoder training steps (mrmt3/packing.py, Trainer(pack_targets=True)): same process, alternating,
device events around each step, graph replay on, bf16, golden-recipe weights.  BASELINE configs[1] MT3Net and MR-MT3
segmem_v2_with_prev at 64 and 12 segments; labels Slakh-shaped (synth_labels(full=False), mean 300) and full-length
(synth_labels(full=True): the packed trainer must take the dense path).  Also reports the per-step length copy (device labels ->
B int32 on the host) and the packed share of the decoder rows.
    python3 profiles/tools/packed_step_ab.py [reps = 5] [segments = 64,12]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "mr-mt3_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np
import torch

from mrmt3 import lib, packing
from mrmt3.synthetic import T5_SMALL, synth_audio, synth_labels
from mrmt3.trainer import Trainer

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SEGS = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "64,12").split(",")]
dev = torch.device("cuda:0")


def model(variant):
    if variant == "t5":
        from models.t5 import T5ForConditionalGeneration
        return T5ForConditionalGeneration(T5_SMALL).load_golden().to(dev)
    from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev
    return T5SegMemV2WithPrev(T5_SMALL, 1, 64).load_golden().to(dev)


def step_ms(tr, audio, lab, prev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tr.train_step(audio, lab, None if prev is None else prev.clone(), audio=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    out = []
    for variant in ("t5", "segmem_v2_with_prev"):
        for B in SEGS:
            audio = torch.from_numpy(synth_audio(B, seed=11)).to(dev)
            prev = torch.from_numpy(synth_labels(B, full=False, seed=13)).to(dev) if variant != "t5" else None
            for kind in ("slakh", "full"):
                lab = torch.from_numpy(synth_labels(B, full=(kind == "full"), seed=12)).to(dev)
                trs = {"dense": Trainer(model(variant), lr=1e-4, graph=True),
                       "packed": Trainer(model(variant), lr=1e-4, graph=True, pack_targets=True)}
                for _ in range(3):                                   # two eager steps + the capture
                    for tr in trs.values():
                        step_ms(tr, audio, lab, prev)
                ms = {k: [] for k in trs}
                for _ in range(REPS):
                    for k, tr in trs.items():
                        ms[k].append(step_ms(tr, audio, lab, prev))
                lengths = packing.row_lengths(lab.cpu().numpy())
                tcap = packing.capacity(lengths, B, 1024)
                t0 = time.perf_counter()
                for _ in range(20):
                    lib.pack_lengths(lab).cpu()
                copy_us = (time.perf_counter() - t0) / 20 * 1e6
                dense, packed = float(np.median(ms["dense"])), float(np.median(ms["packed"]))
                rec = dict(variant=variant, segments=B, labels=kind, T=int(lengths.sum()), Tcap=tcap, dense_rows=B * 1024,
                           dense_ms=round(dense, 3), packed_ms=round(packed, 3), speedup=round(dense / packed, 3),
                           dense_seg_s=round(B / dense * 1e3, 1), packed_seg_s=round(B / packed * 1e3, 1),
                           dense_ms_all=[round(x, 3) for x in ms["dense"]], packed_ms_all=[round(x, 3) for x in ms["packed"]],
                           length_copy_us=round(copy_us, 1))
                print(json.dumps(rec), flush=True)
                out.append(rec)
                for tr in trs.values():
                    tr.close()
    return out


if __name__ == "__main__":
    main()
