"""The row kernels and the fused GEMM epilogues compute the bits they computed before their shared arithmetic moved into
csrc/rowmath.h.  The bitwise tests of the fused forms compare the two forms with each other; both now inline the same
functions, so a slip in one of them (an operand order, an fmaf that became a multiply and an add) would move both together
and the fp64 bound tests allow several ulp.  tests/golden/row_arith_parent.json therefore holds, for each case below, the
sha256 of every output buffer as the PARENT commit (named in the file) wrote it on an MI355X.

How the golden was recorded: the parent commit's csrc/ was built into a library of its own, a script loaded it in place
of the tree's (MRMT3_TOOL_LIB — the C ABI and this binding did not change), ran `run_case(name, dev, lib.set_knob)` for every
name in CASES, calling `lib.reset_knobs()` after each, and dumped {"parent": <commit>, "cases": {name: result}} as JSON.
Inputs come from numpy's default_rng (bf16 by torch's round-to-nearest-even on the host), not from torch's generator."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_arith_parent.json")
BF, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF, "f32": F32}
EPS = 1e-6
STEP = 5                                   # value of the device step counter that salts the masks


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _arr(rng, shape, scale, dtype, dev):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(dtype).to(dev)


def _step(dev):
    return torch.full((1,), STEP, device=dev, dtype=torch.int32)


def _norm_operands(rng, rows, cols, dev):
    x = _arr(rng, (rows, cols), 1.5, F32, dev)
    w = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(cols)).astype(np.float32)).to(dev)
    return x, w


def _rstd(x1):
    x = x1.cpu().numpy().astype(np.float64)
    return torch.from_numpy((1.0 / np.sqrt((x * x).mean(-1) + EPS)).astype(np.float32)).to(x1.device)


# modes of the forward norm: (p, out_drop); of the backward norm: the same with out_drop only under p > 0
FWD_MODES = {"p0": (0.0, False), "p0_drop": (0.0, True), "p0.1": (0.1, False), "p0.1_drop": (0.1, True)}
BWD_MODES = {"p0": (0.0, False), "p0.1": (0.1, False), "p0.1_drop": (0.1, True)}
P_MODES = {"p0": 0.0, "p0.1": 0.1}


def case_norm_fwd(lib, dev, set_knob, cols, y, xn):
    """rows 7: the last workgroup of 4 rows is ragged"""
    rng = np.random.default_rng(101)
    x0, w = _norm_operands(rng, 7, cols, dev)
    yv = None if y == "none" else _arr(rng, (7, cols), 1.0, DT[y], dev)
    out = {}
    for mode, (p, out_drop) in FWD_MODES.items():
        x1, xnv, rstd = lib.add_rmsnorm_fwd(x0, yv, w, EPS, DT[xn], p=p, seed=77, stream_y=3, stream_out=4, out_drop=out_drop,
                                            step=_step(dev))
        out[mode] = {"x1": _sha(x1), "xn": _sha(xnv), "rstd": _sha(rstd)}
    return out


def case_norm_bwd(lib, dev, set_knob, cols, dxn, ri, ro):
    """rows 70: nb_rows gives 4 rows per workgroup, the last one has 2"""
    rng = np.random.default_rng(102)
    x1, w = _norm_operands(rng, 70, cols, dev)
    g = _arr(rng, (70, cols), 1.0, DT[dxn], dev)
    dres = None if ri == "none" else _arr(rng, (70, cols), 1.0, DT[ri], dev)
    dw0 = _arr(rng, (cols,), 0.1, F32, dev)
    rstd = _rstd(x1)
    out = {}
    for mode, (p, out_drop) in BWD_MODES.items():
        dw = dw0.clone()
        dx1, dy = lib.add_rmsnorm_bwd(g, dres, x1, rstd, w, dw, p=p, seed=78, stream_y=5, stream_out=6, out_drop=out_drop,
                                      dx1_dtype=DT[ro], step=_step(dev))
        out[mode] = {"dx1": _sha(dx1), "dy": _sha(dy), "dw": _sha(dw)}
    return out


def _geglu_operands(rng, rows, dff, dtype, dev):
    return _arr(rng, (rows, 2 * dff), 1.0, dtype, dev), _arr(rng, (rows, dff), 1.0, dtype, dev)


def case_geglu_fwd(lib, dev, set_knob, dtype):
    h, _ = _geglu_operands(np.random.default_rng(103), 3, 136, DT[dtype], dev)
    return {mode: {"g": _sha(lib.geglu_fwd(h, p=p, seed=79, stream_id=7, step=_step(dev)))} for mode, p in P_MODES.items()}


def case_geglu_bwd(lib, dev, set_knob, dtype):
    h, dg = _geglu_operands(np.random.default_rng(104), 3, 136, DT[dtype], dev)
    return {mode: {"dh": _sha(lib.geglu_bwd(h, dg, p=p, seed=80, stream_id=8, step=_step(dev)))} for mode, p in P_MODES.items()}


ROWS, K = 72, 128                          # the fused row kernels: one full 64-row tile and a partial one, the smallest K


def _launched(lib, family, fn):
    before = lib.dispatch_counts()[family]
    r = fn()
    assert lib.dispatch_counts()[family] == before + 1, family       # the fused kernel ran, not the two-kernel form
    return r


def case_gemm_addnorm(lib, dev, set_knob, bm):
    set_knob("MRMT3_ROWS_BM", bm)
    rng = np.random.default_rng(105)
    a, wp = _arr(rng, (ROWS, K), 1.0, BF, dev), _arr(rng, (512, K), K ** -0.5, BF, dev)
    x0, wn = _norm_operands(rng, ROWS, 512, dev)
    out = {}
    for mode, (p, out_drop) in FWD_MODES.items():
        x1, xn, rstd = _launched(lib, "gemm_nt_addnorm", lambda: lib.gemm_nt_addnorm(
            a, wp, x0, wn, EPS, p=p, seed=81, stream_y=9, stream_out=10, out_drop=out_drop, step=_step(dev)))
        out[mode] = {"x1": _sha(x1), "xn": _sha(xn), "rstd": _sha(rstd)}
    return out


def case_gemm_normbwd(lib, dev, set_knob, bm, ri, ro):
    set_knob("MRMT3_ROWS_BM", bm)
    rng = np.random.default_rng(106)
    a, wt = _arr(rng, (ROWS, K), 1.0, BF, dev), _arr(rng, (512, K), K ** -0.5, BF, dev)
    x1, wn = _norm_operands(rng, ROWS, 512, dev)
    dres = _arr(rng, (ROWS, 512), 1.0, DT[ri], dev)
    dw0 = _arr(rng, (512,), 0.1, F32, dev)
    rstd = _rstd(x1)
    out = {}
    for mode, p in P_MODES.items():
        dw = dw0.clone()
        dx1, dy = _launched(lib, "gemm_nt_normbwd", lambda: lib.gemm_nt_normbwd(
            a, wt, dres, x1, rstd, wn, dw, p=p, seed=82, stream_y=11, dx1_dtype=DT[ro], step=_step(dev)))
        out[mode] = {"dx1": _sha(dx1), "dy": _sha(dy), "dw": _sha(dw)}
    return out


def case_gemm_geglubwd(lib, dev, set_knob, bm, dff):
    set_knob("MRMT3_ROWS_BM", bm)
    rng = np.random.default_rng(107)
    dy, wt = _arr(rng, (ROWS, K), 1.0, BF, dev), _arr(rng, (dff, K), K ** -0.5, BF, dev)
    h = _arr(rng, (ROWS, 2 * dff), 1.0, BF, dev)
    return {mode: {"dh": _sha(_launched(lib, "gemm_nt_geglubwd", lambda: lib.gemm_nt_geglubwd(
        dy, wt, h, p=p, seed=83, stream_id=12, step=_step(dev))))} for mode, p in P_MODES.items()}


def case_gemm_geglu(lib, dev, set_knob, rows, dff, k):
    """(200, 128, 128): one 128-row tile and a ragged one; (16328, 1024, 128): 512 tiles of 256 rows on a 256-CU device (the
    entry point's own tile rule), the last row tile 200 rows"""
    set_knob("MRMT3_GEGLU_FUSED_MIN_ROWS", 128)
    rng = np.random.default_rng(108)
    x, wi = _arr(rng, (rows, k), 1.0, BF, dev), _arr(rng, (2 * dff, k), k ** -0.5, BF, dev)
    out = {}
    for mode, p in P_MODES.items():
        h, g = _launched(lib, "gemm_nt_geglu", lambda: lib.gemm_nt_geglu(x, wi, p=p, seed=84, stream_id=13, step=_step(dev)))
        out[mode] = {"h": _sha(h), "g": _sha(g)}
    return out


COLS = (256, 512, 1024, 2048)
PAIRS = (("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"))      # residual gradient (in, out)
CASES = {}
for _c in COLS:
    for _y in ("bf16", "f32") + (("none",) if _c == 512 else ()):
        for _xn in ("bf16", "f32"):
            CASES["norm_fwd-c%d-y_%s-xn_%s" % (_c, _y, _xn)] = (case_norm_fwd, (_c, _y, _xn))
    for _g in ("bf16", "f32"):
        for _ri, _ro in PAIRS if _c == 512 else PAIRS[:1]:       # a bf16 residual gradient exists at the model width only
            CASES["norm_bwd-c%d-dxn_%s-res_%s_%s" % (_c, _g, _ri, _ro)] = (case_norm_bwd, (_c, _g, _ri, _ro))
CASES["norm_bwd-c512-dxn_bf16-res_none_f32"] = (case_norm_bwd, (512, "bf16", "none", "f32"))
for _d in ("bf16", "f32"):
    CASES["geglu_fwd-%s" % _d] = (case_geglu_fwd, (_d,))
    CASES["geglu_bwd-%s" % _d] = (case_geglu_bwd, (_d,))
for _bm in (64, 128):
    CASES["gemm_addnorm-tile%d" % _bm] = (case_gemm_addnorm, (_bm,))
    for _ri, _ro in PAIRS:
        CASES["gemm_normbwd-tile%d-res_%s_%s" % (_bm, _ri, _ro)] = (case_gemm_normbwd, (_bm, _ri, _ro))
    for _dff in (512, 1024):
        CASES["gemm_geglubwd-tile%d-dff%d" % (_bm, _dff)] = (case_gemm_geglubwd, (_bm, _dff))
CASES["gemm_geglu-tile128"] = (case_gemm_geglu, (200, 128, 128))
CASES["gemm_geglu-tile256"] = (case_gemm_geglu, (16328, 1024, 128))


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
def test_row_arithmetic_bits_equal_the_parent(dev, golden, knobs, name):
    got = run_case(name, dev, knobs.set)
    assert got == golden["cases"][name]
    # dropout reaches the outputs: a p = 0.1 mode differs from its p = 0 twin — except where nothing is masked at all
    # (no y to drop and the output not dropped), which must then BE the twin
    for mode in got:
        if not mode.startswith("p0.1"):
            continue
        twin = got["p0" + mode[len("p0.1"):]] if "p0" + mode[len("p0.1"):] in got else got["p0"]
        if "-y_none-" in name and mode == "p0.1":
            assert got[mode] == twin
        else:
            assert got[mode] != twin, mode
