"""The bf16 attention kernels (csrc/attention.hip: forward, dQ, dK/dV, dense and packed; csrc/attention_onepass.hip) write
the bits they wrote before their row prologue, K/V staging, pair loop, quad dropout mask, row store and launch ladders were
folded into one copy each (csrc/attn_common.h, attn_launch).  The integer-operand tests (tests/test_exact_gpu.py) are exact
under ANY summation order; the operands here are real-valued, so a reordered sum, a tile taken from the wrong offset or a mask
word taken from the wrong lane shows.  tests/golden/attn_parent.json holds, for each case below, the sha256 of every output
buffer as the PARENT commit (named in the file) wrote it on an MI355X.

How the golden was recorded: the parent commit's csrc/ was built into a library of its own, a script loaded it in place of
the tree's (MRMT3_TOOL_LIB — the C ABI and this binding did not change), ran `run_case(name, dev, lib.set_knob)` for every
name in CASES, calling `lib.reset_knobs()` after each, and dumped {"parent": <commit>, "cases": {name: result}} as JSON.
Inputs come from numpy's default_rng (bf16 by torch's round-to-nearest-even on the host), not from torch's generator.

Every case runs with p = 0 and p = 0.1 (device step counter 5, the low half of O written and read back), through the C ABI
with caller-owned outputs pre-filled with a fixed value — an element nobody writes hashes the same on both sides — and
asserts its kernel family through lib.dispatch_counts().  RT (64- or 128-row tiles) and PAIR do not change a row's
arithmetic: that the same INSTANTIATIONS run is checked by a kernel trace of this file (profiles/r20_attn_fold.txt, C)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_parent.json")
BF, F32 = torch.bfloat16, torch.float32
H, W = 6, 6 * 64
STEP = 5                                   # value of the device step counter that salts the dropout mask
SEED, STREAM = 85, 14
FILL = 0.375                               # what every output buffer holds before the launch
LENGTHS, TCAP = (0, 200, 37, 64), 384      # the packed cases: T = 301, the tail rows 301 .. 383 belong to two surplus entries


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _arr(rng, shape, scale, dev, dtype=BF):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(dtype).to(dev)


def _fill(shape, dtype, dev):
    return torch.full(shape, FILL, dtype=dtype, device=dev)


def _launched(lib, fn, **families):
    before = lib.dispatch_counts()
    fn()
    after = lib.dispatch_counts()
    for fam in ("attn_fwd", "attn_bwd", "attn_bwd_onepass", "attn_fwd_varlen", "attn_bwd_varlen", "attn_f32"):
        assert after[fam] == before[fam] + families.get(fam, 0), (fam, before[fam], after[fam])


def _step(dev):
    return torch.full((1,), STEP, device=dev, dtype=torch.int32)


def _dense(lib, dev, q, k, v, d_o, B, Lq, Lk, causal, bwd_family, ldo=W, grads=None):
    """forward (+ backward when d_o is given) at p = 0 and p = 0.1 -> {p: {buffer: sha256}}.  `grads`: (dq, dk, dv) views to
    write into (hashed through `grads_buf`), else contiguous buffers."""
    L, p_, s_ = lib.load(), lib._p, lib._stream
    step, out = _step(dev), {}
    for tag, p in (("p0", 0.0), ("p0.1", 0.1)):
        obuf, lobuf = _fill((B * Lq, ldo), BF, dev), _fill((B * Lq, ldo), BF, dev)
        o, o_lo, lse = obuf[:, :W], lobuf[:, :W], _fill((B, H, Lq), F32, dev)
        _launched(lib, lambda: lib._check(L.mrmt3_attn_fwd(
            p_(q), q.stride(0), p_(k), k.stride(0), p_(v), v.stride(0), p_(o), ldo, p_(o_lo), p_(lse), B, H, Lq, Lk, int(causal),
            lib.BF16, p, SEED, p_(step), STREAM, s_()), "attn_fwd"), attn_fwd=1)
        r = {"o": _sha(obuf), "o_lo": _sha(lobuf), "lse": _sha(lse)}
        if d_o is not None:
            if grads is None:
                gbuf = None
                dq, dk, dv = _fill((B * Lq, W), BF, dev), _fill((B * Lk, W), BF, dev), _fill((B * Lk, W), BF, dev)
            else:
                gbuf = _fill(grads, BF, dev)
                dq, dk, dv = gbuf[:, :W], gbuf[:, W:2 * W], gbuf[:, 2 * W:]
            delta = _fill((B, H, Lq), F32, dev)
            _launched(lib, lambda: lib._check(L.mrmt3_attn_bwd(
                p_(q), q.stride(0), p_(k), k.stride(0), p_(v), v.stride(0), p_(o), ldo, p_(o_lo), p_(d_o), d_o.stride(0),
                p_(lse), p_(delta), p_(dq), dq.stride(0), p_(dk), dk.stride(0), p_(dv), dv.stride(0), B, H, Lq, Lk,
                int(causal), p, SEED, p_(step), STREAM, s_()), "attn_bwd"), **{bwd_family: 1})
            r["delta"] = _sha(delta)
            if gbuf is None:
                r.update(dq=_sha(dq), dk=_sha(dk), dv=_sha(dv))
            else:
                r["dq_dk_dv"] = _sha(gbuf)
        out[tag] = r
    return out


def case_dense(lib, dev, set_knob, B, Lq, Lk, causal, knobs, bwd_family, seed):
    """Dense rows, contiguous operands.  (2, 200, 200, causal): ragged last tiles; 64-row tiles by default (RT = 1), 128-row
    unpaired tiles with MRMT3_ATTN_FINE=0 (RT = 2).  (2, 200, 320, cross, MRMT3_ATTN_ONEPASS=0): the two-pass kernels with a
    ragged last key tile.  (43, 300, 300, causal): n = 3 tiles in 2 pair workgroups, 516 >= 512 of them: paired, the odd middle
    tile takes the pass-1 break.  (2, 100, 256 / 290, cross, MRMT3_ATTN_ONEPASS_MIN_BH=12): the one-pass backward, NT = 2, and
    NT = 3 with ragged keys; the last query block is ragged in both."""
    for name, value in knobs:
        set_knob(name, value)
    rng = np.random.default_rng(seed)
    q, k, v = _arr(rng, (B * Lq, W), 0.35, dev), _arr(rng, (B * Lk, W), 1.0, dev), _arr(rng, (B * Lk, W), 1.0, dev)
    d_o = _arr(rng, (B * Lq, W), 1.0, dev)
    return _dense(lib, dev, q, k, v, d_o, B, Lq, Lk, causal, bwd_family)


def case_strided(lib, dev, set_knob, ldo, backward):
    """q, k, v are columns 0:384, 384:768, 768:1152 of one [B * L, 1152] buffer (causal, B = 2, L = 200); dq, dk, dv the same
    columns of one gradient buffer.  ldo = 388, forward only: rows that are not 16-byte aligned take the 8-byte store path."""
    B, Lq = 2, 200
    rng = np.random.default_rng(307)
    qkv = _arr(rng, (B * Lq, 3 * W), 1.0, dev)
    qkv[:, :W] *= 0.35
    d_o = _arr(rng, (B * Lq, W), 1.0, dev) if backward else None
    return _dense(lib, dev, qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], d_o, B, Lq, Lq, True, "attn_bwd", ldo=ldo,
                  grads=(B * Lq, 3 * W))


def case_packed(lib, dev, set_knob, Lk):
    """Packed rows of lengths LENGTHS at capacity TCAP.  Lk = 0: causal self-attention (keys packed like the queries).
    Lk = 320 / 100: cross-attention over dense keys; the empty row takes the Lq = 0 path of dK/dV.  The tail rows of every
    packed output are zeroed by the surplus entries."""
    L, p_, s_ = lib.load(), lib._p, lib._stream
    B, Lmax = len(LENGTHS), 256
    lab = np.full((B, Lmax), -100, dtype=np.int64)
    for b, n in enumerate(LENGTHS):
        lab[b, :n] = 3 + (np.arange(n) * 7 + b) % 1000
    plan = lib.pack_plan(torch.from_numpy(lab).to(dev), TCAP, 0, 0)
    rng = np.random.default_rng(308 + Lk)
    rows_k = TCAP if Lk == 0 else B * Lk
    q, k, v = _arr(rng, (TCAP, W), 0.35, dev), _arr(rng, (rows_k, W), 1.0, dev), _arr(rng, (rows_k, W), 1.0, dev)
    d_o = _arr(rng, (TCAP, W), 1.0, dev)
    step, out = _step(dev), {}
    for tag, p in (("p0", 0.0), ("p0.1", 0.1)):
        o, o_lo, lse = _fill((TCAP, W), BF, dev), _fill((TCAP, W), BF, dev), _fill((H, TCAP), F32, dev)
        _launched(lib, lambda: lib._check(L.mrmt3_attn_fwd_varlen(
            p_(q), W, p_(k), W, p_(v), W, p_(o), W, p_(o_lo), p_(lse), p_(plan.row_off), p_(plan.tiles), B, H, TCAP, Lmax, Lk,
            int(Lk == 0), lib.BF16, p, SEED, p_(step), STREAM, s_()), "attn_fwd_varlen"), attn_fwd_varlen=1)
        dq, dk, dv = _fill((TCAP, W), BF, dev), _fill((rows_k, W), BF, dev), _fill((rows_k, W), BF, dev)
        delta = _fill((H, TCAP), F32, dev)
        _launched(lib, lambda: lib._check(L.mrmt3_attn_bwd_varlen(
            p_(q), W, p_(k), W, p_(v), W, p_(o), W, p_(o_lo), p_(d_o), W, p_(lse), p_(delta), p_(dq), W, p_(dk), W, p_(dv), W,
            p_(plan.row_off), p_(plan.tiles), B, H, TCAP, Lmax, Lk, int(Lk == 0), lib.BF16, p, SEED, p_(step), STREAM, s_()),
            "attn_bwd_varlen"), attn_bwd_varlen=1)
        assert int(plan.err.item()) == 0
        out[tag] = {"o": _sha(o), "o_lo": _sha(o_lo), "lse": _sha(lse), "delta": _sha(delta), "dq": _sha(dq), "dk": _sha(dk),
                    "dv": _sha(dv)}
    return out


FINE0, TWOPASS = ("MRMT3_ATTN_FINE", 0), ("MRMT3_ATTN_ONEPASS", 0)
ONEPASS = ("MRMT3_ATTN_ONEPASS_MIN_BH", 12)
CASES = {
    "dense-causal-2x200-rt1": (case_dense, (2, 200, 200, True, (), "attn_bwd", 301)),
    "dense-causal-2x200-rt2": (case_dense, (2, 200, 200, True, (FINE0,), "attn_bwd", 301)),
    "dense-cross-2x200x320-rt1": (case_dense, (2, 200, 320, False, (TWOPASS,), "attn_bwd", 302)),
    "dense-cross-2x200x320-rt2": (case_dense, (2, 200, 320, False, (TWOPASS, FINE0), "attn_bwd", 302)),
    "paired-causal-43x300": (case_dense, (43, 300, 300, True, (), "attn_bwd", 303)),
    "onepass-2x100x256-nt2": (case_dense, (2, 100, 256, False, (ONEPASS,), "attn_bwd_onepass", 304)),
    "onepass-2x100x290-nt3": (case_dense, (2, 100, 290, False, (ONEPASS,), "attn_bwd_onepass", 305)),
    "strided-causal-2x200": (case_strided, (W, True)),
    "strided-causal-2x200-ldo388-fwd": (case_strided, (388, False)),
    "packed-self-causal": (case_packed, (0,)),
    "packed-cross-320": (case_packed, (320,)),
    "packed-cross-100": (case_packed, (100,)),
}


def run_case(name, dev, set_knob):
    from mrmt3 import lib
    fn, args = CASES[name]
    out = fn(lib, dev, set_knob, *args)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_golden_names_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES) and len(golden["parent"]) == 40


@pytest.mark.parametrize("name", sorted(CASES))
def test_attn_bits_equal_the_parent(dev, golden, knobs, name):
    got = run_case(name, dev, knobs.set)
    assert got == golden["cases"][name]
    # dropout leaves the softmax statistics alone and reaches every other buffer (the one-pass backward keeps delta in LDS:
    # its buffer still holds the fill)
    same = {"lse", "delta"} if name.startswith("onepass") else {"lse"}
    for key in got["p0"]:
        assert (got["p0.1"][key] == got["p0"][key]) == (key in same), key
