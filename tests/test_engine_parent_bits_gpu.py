"""Engine.forward / Engine.backward write the bits they wrote before mrmt3/engine.py stated each sublayer once (the attention
site, the feed-forward sublayer, the closing norm and the input prologue as shared pieces; the one-layer memory-encoder shortcut
composed from them).  No kernel changed: what this file pins is the wiring — which launches a step is made of, with which
operands, dropout site ids and output dtypes.  tests/golden/engine_parent.json holds, for each case below, the sha256 of the
forward output and of every tensor of flat.G (by state-dict key) as the PARENT commit (named in the file) wrote them on an
MI355X, and the lib.dispatch_counts() delta of the case.

How the golden was recorded (profiles/r27_engine_sublayers.txt): the parent commit's tree was exported with `git archive`,
its mr-mt3_amd put first on sys.path with MRMT3_TOOL_LIB naming the one built library (csrc/ is unchanged), and a script ran
`run_case(name, dev)` of this file for every name in CASES in two separate processes; a buffer is pinned only where both
processes hashed it alike (one that the parent itself does not reproduce is named under "unpinned" and left to the tolerances
of tests/test_model_gpu.py).  The golden is never re-recorded from the code under test.

Every case: dict(T5_SMALL, num_layers=2, num_decoder_layers=2) with the golden weights, B = 2, synth_mel(2), 256 Slakh-shaped
labels; the engine is driven directly (site counter restarted, no device step counter), the backward from seeded dlogits — no
cross-entropy, whose f64 loss sum depends on the arrival order of its workgroups.  Each case is the smallest that takes its
branch: the in-place residual path (no tape), dense / packed rows, the f32 engine, the memory encoder prepended (v1), as extra
cross-attention keys (v2), fed from targets_prev (with_prev), and the generic multi-layer memory path (segmem_num_layers=2)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_parent.json")
BF, F32 = torch.bfloat16, torch.float32
B, L = 2, 256

#        name                              variant                dtype  p    packed  memory layers  grad
CASES = {
    "t5-bf16-eval-states":                ("t5",                  BF,    0.0, False,  0,             False),
    "t5-bf16-p0.1":                       ("t5",                  BF,    0.1, False,  0,             True),
    "t5-bf16-p0.1-packed":                ("t5",                  BF,    0.1, True,   0,             True),
    "t5-f32-p0.1":                        ("t5",                  F32,   0.1, False,  0,             True),
    "segmem_v1-bf16-p0.1":                ("segmem_v1",           BF,    0.1, False,  1,             True),
    "segmem_v2-bf16-p0.1":                ("segmem_v2",           BF,    0.1, False,  1,             True),
    "segmem_v2_with_prev-bf16-p0.1-packed": ("segmem_v2_with_prev", BF,  0.1, True,   1,             True),
    "segmem_v2_with_prev-f32-p0":         ("segmem_v2_with_prev", F32,   0.0, False,  1,             True),
    "segmem_v2-bf16-p0.1-mem2":           ("segmem_v2",           BF,    0.1, False,  2,             True),
}
# The one accepted difference from the parent: the bf16 one-layer memory-encoder shortcut now goes through _proj_geglu_bwd like
# the stacks, so (MRMT3_FUSE_ROWS bit 4, the default) its wo data gradient [B*64, 512] x [1024, 512]^T and the gated-GELU
# backward behind it are the one gemm_nt_geglubwd launch — same bits, tests/test_gemm_rows_gpu.py — instead of a plain NT
# product (128 rows: the tile kernel) and the row kernel.  (segmem_v1 takes the same shortcut as the two v2 cases.)
FUSED_SHORTCUT = ("segmem_v1-bf16-p0.1", "segmem_v2-bf16-p0.1", "segmem_v2_with_prev-bf16-p0.1-packed")
_MODELS = {}


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _model(variant, dtype, mem_layers, dev):
    key = (variant, dtype, mem_layers)
    if key not in _MODELS:
        from models.t5 import T5ForConditionalGeneration
        from models.t5_segmem import T5SegMem
        from models.t5_segmem_v2 import T5SegMemV2
        from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev
        from mrmt3.synthetic import T5_SMALL
        cls = {"t5": T5ForConditionalGeneration, "segmem_v1": T5SegMem, "segmem_v2": T5SegMemV2,
               "segmem_v2_with_prev": T5SegMemV2WithPrev}[variant]
        cfg = dict(T5_SMALL, num_layers=2, num_decoder_layers=2)
        m = cls(cfg, compute_dtype=dtype) if variant == "t5" else cls(cfg, segmem_num_layers=mem_layers, segmem_length=64,
                                                                      compute_dtype=dtype)
        _MODELS[key] = m.load_golden().to(dev)
    return _MODELS[key]


def run_case(name, dev):
    from mrmt3 import lib, packing
    from mrmt3.synthetic import synth_labels, synth_mel
    variant, dtype, p, packed, mem_layers, grad = CASES[name]
    m = _model(variant, dtype, mem_layers, dev)
    eng, flat = m.engine, m.flat
    assert eng.cfg["dropout_rate"] == 0.1
    mel = torch.from_numpy(synth_mel(B)).to(dev)
    lab = synth_labels(B, L, full=False, seed=777, mean_len=120)
    labels = torch.from_numpy(lab).to(dev)
    prev = torch.from_numpy(synth_labels(B, L, full=False, seed=999, mean_len=120)).to(dev)      # (filled in place: a fresh copy)
    plan = None
    if packed:
        tcap = packing.capacity(packing.row_lengths(lab), B, L)       # (290 scored rows, Tcap 512: a tail of empty rows)
        plan = lib.pack_plan(labels.contiguous(), tcap, eng.cfg["decoder_start_token_id"], eng.cfg["pad_token_id"])
    eng._stream_ctr, eng.step_dev = 0, None
    torch.cuda.synchronize()
    lib.dispatch_counts(reset=True)
    out, tape = eng.forward(mel, labels, prev if variant == "segmem_v2_with_prev" else None, training=p > 0.0, need_grad=grad,
                            want_logits=grad, pack=plan)
    r = {"out": _sha(out)}
    if grad:
        flat.ensure_grads()
        flat.G.zero_()
        rows = out.numel() // eng.V
        dl = torch.from_numpy((np.random.default_rng(2701).standard_normal((rows, eng.V)) * 0.01).astype(np.float32))
        eng.backward(tape, dl.to(dev).to(dtype).contiguous())
        torch.cuda.synchronize()
        r["grads"] = {k: _sha(flat.grad(k)) for k in flat.shapes}
    else:
        assert tape is None
    torch.cuda.synchronize()
    r["counts"] = {k: v for k, v in lib.dispatch_counts().items() if v}
    return r


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_the_golden_names_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    for name, c in golden["cases"].items():
        assert "out" in c and (not CASES[name][5] or len(c["grads"]) >= 51), name       # (a 2 + 2 layer T5 has 51 tensors)


@pytest.mark.parametrize("name", list(CASES))
def test_bits_and_launches_equal_the_parent(dev, golden, name):
    want = golden["cases"][name]
    got = run_case(name, dev)
    counts = dict(want["counts"])
    if name in FUSED_SHORTCUT:
        counts["gemm_nt_geglubwd"] = counts.get("gemm_nt_geglubwd", 0) + 1
        counts["gemm_nt_tile"] -= 1
    assert got["counts"] == counts
    assert got["out"] == want["out"]
    if "grads" in want:
        unpinned = set(golden.get("unpinned", {}).get(name, []))
        assert set(want["grads"]) | unpinned == set(got["grads"])
        differ = [k for k, h in want["grads"].items() if got["grads"][k] != h]
        assert not differ, differ
