"""The ping-pong GEMMs (csrc/gemm8.hip: NT, split K, fused wi + GEGLU; csrc/gemm_tn8.hip: TN single and grouped) write the
bits they wrote before their K loop moved into csrc/pingpong.h and their LDS-DMA primitives into csrc/lds_dma.h.  The
integer-operand tests (tests/test_exact_gpu.py) are exact under ANY summation order, so they cannot see an accumulation that
was reordered (a phase's MFMAs issued in another order, a K step skipped into the next buffer): the operands here are
real-valued.  tests/golden/pingpong_parent.json holds, for each case below, the sha256 of every output buffer as the PARENT
commit (named in the file) wrote it on an MI355X.

How the golden was recorded: the parent commit's csrc/ was built into a library of its own, a script loaded it in place of
the tree's (MRMT3_TOOL_LIB — the C ABI and this binding did not change), ran `run_case(name, dev, lib.set_knob)` for every
name in CASES, calling `lib.reset_knobs()` after each, and dumped {"parent": <commit>, "cases": {name: result}} as JSON.
Inputs come from numpy's default_rng (bf16 by torch's round-to-nearest-even on the host), not from torch's generator.

Tile heights below are those of a 256-CU device (the plan of csrc/gemm8.hip: 128-row tiles while the 256-row tiles do not
fill the chip); each case asserts through lib.dispatch_counts() that the intended kernel family ran."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _exact as ex  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pingpong_parent.json")
BF, F32 = torch.bfloat16, torch.float32
STEP = 5                                   # value of the device step counter that salts the dropout mask


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _arr(rng, shape, scale, dtype, dev):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(dtype).to(dev)


def _launched(lib, fn, **families):
    before = lib.dispatch_counts()
    r = fn()
    after = lib.dispatch_counts()
    for fam, n in families.items():
        assert after[fam] == before[fam] + n, (fam, before[fam], after[fam])
    return r


def _nt_knobs(set_knob):
    set_knob("MRMT3_GEMM8_ALL", 1)
    set_knob("MRMT3_GEMM8_MIN_M", 128)


def _nt_outputs(lib, rng, a, b, modes, dev, family):
    M, N = a.shape[0], b.shape[0]
    out = {}
    for mode in modes:
        if mode == "bf16":
            c = _launched(lib, lambda: lib.gemm_nt(a, b, out_dtype=BF), **{family: 1})
        elif mode == "f32":
            c = _launched(lib, lambda: lib.gemm_nt(a, b, out_dtype=F32), **{family: 1})
        else:
            c = _arr(rng, (M, N), 1.0, F32, dev)
            _launched(lib, lambda: lib.gemm_nt(a, b, out=c, accumulate=True), **{family: 1})
        out[mode] = _sha(c)
    return out


def case_nt(lib, dev, set_knob, M, N, K, modes):
    """(300, 384, K): 128-row tiles, ragged last row tile, shifted last column tile; K = 128: a tile's first and last K step
    are adjacent, 384: with a middle step.  (16130, 1152, K): 64 x 5 = 320 tiles of 256 rows on 256 workgroups — some run
    two tiles, and the store batches of one tile drain under the next tile's first K step; K = 128: nk == 2."""
    _nt_knobs(set_knob)
    rng = np.random.default_rng(201)
    a, b = _arr(rng, (M, K), 1.0, BF, dev), _arr(rng, (N, K), K ** -0.5, BF, dev)
    return _nt_outputs(lib, rng, a, b, modes, dev, "gemm_nt8")


def case_nt_strided(lib, dev, set_knob):
    """A = columns 384:768 of a [300, 1152] buffer (lda = 1152, K = 384), N = 512"""
    _nt_knobs(set_knob)
    rng = np.random.default_rng(202)
    abuf, b = _arr(rng, (300, 1152), 1.0, BF, dev), _arr(rng, (512, 384), 384 ** -0.5, BF, dev)
    return _nt_outputs(lib, rng, abuf[:, 384:768], b, ("bf16", "f32", "f32_acc"), dev, "gemm_nt8")


def case_splitk(lib, dev, set_knob):
    """(1100, 512, 2048) through mrmt3_gemm_nt_ws: 18 tiles of 128 rows x 4 K ranges, the slab path and its reduce"""
    rng = np.random.default_rng(203)
    a, b = _arr(rng, (1100, 2048), 1.0, BF, dev), _arr(rng, (512, 2048), 2048 ** -0.5, BF, dev)
    return _nt_outputs(lib, rng, a, b, ("bf16", "f32"), dev, "gemm_nt_splitk")


def case_geglu256(lib, dev, set_knob):
    """rows 8100, dff 1024, K 128: 32 x 8 = 256 tiles of 256 rows (the entry point's own tile rule), the last row tile 164
    rows.  (The 128-row tile of this launch: tests/test_row_arith_parent_bits_gpu.py.)"""
    rng = np.random.default_rng(204)
    x, wi = _arr(rng, (8100, 128), 1.0, BF, dev), _arr(rng, (2048, 128), 128 ** -0.5, BF, dev)
    step = torch.full((1,), STEP, device=dev, dtype=torch.int32)
    out = {}
    for mode, p in (("p0", 0.0), ("p0.1", 0.1)):
        h, g = _launched(lib, lambda: lib.gemm_nt_geglu(x, wi, p=p, seed=85, stream_id=14, step=step), gemm_nt_geglu=1)
        out[mode] = {"h": _sha(h), "g": _sha(g)}
    return out


def case_tn(lib, dev, set_knob):
    """(8200, 896, 320): 4 x 2 tiles, both last tiles shifted, token ranges of which the last is ragged"""
    set_knob("MRMT3_TN8_ALL", 1)
    rng = np.random.default_rng(205)
    a, b = _arr(rng, (8200, 896), 1.0, BF, dev), _arr(rng, (8200, 320), 1.0, BF, dev)
    c0 = _arr(rng, (896, 320), 1.0, F32, dev)
    out = {}
    for mode, acc in (("overwrite", False), ("accumulate", True)):
        c = c0.clone()
        _launched(lib, lambda: lib.gemm_tn(a, b, c, accumulate=acc), tn8=1)
        out[mode] = _sha(c)
    return out


def case_tn_group(lib, dev, set_knob):
    """the four sites of tests/_exact.py, accumulate and overwrite mixed as in tests/test_exact_gpu.py"""
    rng = np.random.default_rng(206)
    grp, outs = lib.TnGroup(), []
    for i, (M, N1, N2) in enumerate(ex.TN_GROUP_SITES):
        a, b = _arr(rng, (M, N1), 1.0, BF, dev), _arr(rng, (M, N2), 1.0, BF, dev)
        c = _arr(rng, (N1, N2), 1.0, F32, dev)
        assert lib.TnGroup.ok(a, b, c)
        grp.add(a, b, c, accumulate=i % 2 == 0)
        outs.append(c)
    _launched(lib, grp.flush, tn_group=1)
    return {"site%d" % i: _sha(c) for i, c in enumerate(outs)}


ALL3 = ("bf16", "f32", "f32_acc")
CASES = {
    "nt-tile128-300x384x128": (case_nt, (300, 384, 128, ALL3)),
    "nt-tile128-300x384x384": (case_nt, (300, 384, 384, ALL3)),
    "nt-tile256-16130x1152x256": (case_nt, (16130, 1152, 256, ALL3)),
    "nt-tile256-16130x1152x128": (case_nt, (16130, 1152, 128, ("f32",))),
    "nt-strided-300x512x384": (case_nt_strided, ()),
    "splitk-1100x512x2048": (case_splitk, ()),
    "geglu-tile256-8100x1024x128": (case_geglu256, ()),
    "tn-8200x896x320": (case_tn, ()),
    "tn-group": (case_tn_group, ()),
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


@pytest.mark.parametrize("name", sorted(CASES))
def test_pingpong_bits_equal_the_parent(dev, golden, knobs, name):
    got = run_case(name, dev, knobs.set)
    assert got == golden["cases"][name]
    if name.startswith("geglu"):
        assert got["p0.1"]["g"] != got["p0"]["g"] and got["p0.1"]["h"] == got["p0"]["h"]     # the mask reaches g only
