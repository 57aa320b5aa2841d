"""The optimizer tail computes the bits it computed before the AdamW and gradient-norm siblings were folded into
mrmt3_adamw_step / mrmt3_grad_norm: tests/golden/optimizer_tail_parent.json holds, for each case below, the sha256 of every
output buffer and the three `stat` floats as bit patterns, recorded with the three AdamW kernels and two norm kernels of
library version 120 on an MI355X.  Inputs come from numpy's default_rng, so they do not depend on torch's generator."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizer_tail_parent.json")

N = 9216                                   # 2303 / 2304 16-byte groups: 2.25 chunks of the range kernel, the last one ragged
RANGES = [(0, 4, 0.0, 1.0), (8, 5000, 0.01, 0.5), (5000, N, 0.1, 2.0)]   # a hole at [4, 8); range 1 spans the chunk boundary
CLIP = dict(stat=[1.0, 0.37, 0.0], clip_value=0.2)
ADAMW_CASES = {                            # name -> (stat, clip_value, ranges, ema_decay)
    "a_flat": (None, 0.0, None, 0.0),
    "b_flat_clip": (CLIP["stat"], CLIP["clip_value"], None, 0.0),
    "c_flat_skip": ([1.0, 0.37, 1.0], 0.0, None, 0.0),
    "d_ranges": (None, 0.0, RANGES, 0.0),
    "e_ranges_clip_ema": (CLIP["stat"], CLIP["clip_value"], RANGES, 0.9),
}
STRIDE4 = 2048 * 256                       # groups one sweep of the norm's fixed grid covers
NORM_N = 4 * (3 * STRIDE4 + 1000)          # lanes below 1000 run the four-strides loop, the others the tail loop
NORM_RANGES = [(0, 4000, 0.0, 1.0), (4004, 4000000, 0.0, 1.0), (4000008, NORM_N, 0.0, 1.0)]   # holes of 1 and 2 groups
NORM_CASES = {                             # name -> (n, seed, ranges, index of a planted inf)
    "flat": (NORM_N, 21, None, None),
    "ranges": (NORM_N, 21, NORM_RANGES, None),
    "inf": (4096, 22, None, 1234),
}


def _sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _f32_hex(t):
    return ["%08x" % int(x) for x in t.detach().cpu()[:3].numpy().view(np.uint32)]


def new_api_adamw(lib, p, g, m, v, lr, step, grad_scale, shadow, stat, clip_value, ranges, ema, ema_decay):
    lib.adamw_step(p, g, m, v, lr, step, grad_scale=grad_scale, shadow=shadow, stat=stat, clip_value=clip_value,
                   ranges=ranges, ema=ema, ema_decay=ema_decay)


def new_api_norm(lib, g, grad_scale, max_norm, skip_nonfinite, ws, stat, skipped, ranges):
    lib.grad_norm(g, grad_scale, max_norm, skip_nonfinite, ws, stat, skipped, ranges=ranges)


def run_adamw_case(name, dev, adamw=new_api_adamw):
    """Two consecutive steps (a fresh gradient each) of one configuration; the hashes of every buffer after each."""
    from mrmt3 import lib
    stat_v, clip_value, ranges, ema_decay = ADAMW_CASES[name]
    rng = np.random.default_rng(11)
    f = lambda scale=1.0: torch.from_numpy((rng.standard_normal(N) * scale).astype(np.float32)).to(dev)
    p, m, v, ema, g1, g2 = f(0.1), f(0.01), f(1e-3).abs(), f(0.1), f(), f()
    shadow = torch.zeros(N, device=dev, dtype=torch.bfloat16)
    lr = torch.full((1,), 1e-3, device=dev)
    step = torch.full((1,), 3, device=dev, dtype=torch.int32)
    stat = None if stat_v is None else torch.tensor(stat_v + [0.0], device=dev)
    tab = None if ranges is None else lib.OptRanges(ranges, N).to(dev)
    before = [t.clone() for t in (p, m, v, shadow, ema)]
    out = {}
    for k, g in enumerate((g1, g2)):
        adamw(lib, p, g, m, v, lr, step, 1.0 / 3, shadow, stat, clip_value, tab, ema if ema_decay else None, ema_decay)
        torch.cuda.synchronize()
        out["step%d" % (k + 1)] = {"p": _sha(p), "m": _sha(m), "v": _sha(v), "shadow": _sha(shadow), "ema": _sha(ema),
                                   "step_dev": int(step.item())}
    if stat is not None:
        out["stat"] = _f32_hex(stat)
    changed = [not torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, (p, m, v, shadow, ema))]
    return out, changed


def run_norm_case(name, dev, norm=new_api_norm):
    from mrmt3 import lib
    n, seed, ranges, inf_at = NORM_CASES[name]
    g = torch.from_numpy(np.random.default_rng(seed).standard_normal(n, dtype=np.float32)).to(dev)
    if inf_at is not None:
        g[inf_at] = float("inf")
    tab = None if ranges is None else lib.OptRanges(ranges, n).to(dev)
    ws = lib.grad_norm_workspace(dev).zero_()
    stat, skipped = torch.full((4,), -7.0, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
    norm(lib, g, 0.5, 1.0, True, ws, stat, skipped, tab)
    torch.cuda.synchronize()
    return {"stat": _f32_hex(stat), "skipped": int(skipped.item()), "partials": _sha(ws)}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(ADAMW_CASES))
def test_adamw_step_bits_equal_the_three_kernels_it_replaced(dev, golden, name):
    got, changed = run_adamw_case(name, dev)
    assert got == golden["adamw"][name]
    assert got["step2"]["step_dev"] == 5
    ema_on = bool(ADAMW_CASES[name][3])
    if name == "c_flat_skip":
        assert changed == [False] * 5                       # a skipped step: nothing but the step counter moves
    else:
        assert changed == [True, True, True, True, ema_on]


@pytest.mark.parametrize("name", sorted(NORM_CASES))
def test_grad_norm_bits_equal_the_two_kernels_it_replaced(dev, golden, name):
    got = run_norm_case(name, dev)
    assert got == golden["norm"][name]
    stat = np.array([int(h, 16) for h in got["stat"]], dtype=np.uint32).view(np.float32)
    if name == "inf":
        assert np.isinf(stat[0]) and stat[1] == 0.0 and stat[2] == 1.0 and got["skipped"] == 1
    else:
        assert np.isfinite(stat[0]) and 0.0 < stat[1] < 1.0 and stat[2] == 0.0 and got["skipped"] == 0
