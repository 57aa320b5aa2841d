"""Per-bin tests of the log-mel kernels (csrc/logmel.hip) on a real MI355X: every element of every case against the fp64
restatement of the header's contract, held to the linear-domain bound of tests/_exact_logmel.py (constructions, reference,
K and R and their derivation live there; tests/test_exact_logmel_cpu.py proves them without a GPU).

Every call goes through the raw C ABI into a view of a larger buffer pre-filled with a sentinel (the rows before and behind
the view must stay untouched), asserts through the dispatch counters which kernel took it, and is repeated with bf16 output,
which must be round-to-nearest-even of the f32 output of the same call and kernel, bit for bit.  A case the wave kernel takes
is run through the general kernel too (MRMT3_LOGMEL=0)."""
import numpy as np
import pytest
import torch

import _exact_logmel as xl

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 4096                      # elements before and behind the output view (a multiple of 16 bytes in f32 and bf16)
CASES = {c["name"]: c for c in xl.small_cases()}
_REFS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from mrmt3 import lib
    lib.load()
    return torch.device("cuda:0")


def _ref(c):
    if c["name"] not in _REFS:
        _REFS[c["name"]] = xl.reference(c)
    return _REFS[c["name"]]


def _launch(c, dev, bf16, kernel, misalign=False):
    """One call of the entry point the case names; returns the output as numpy (f32, or the bf16 bit patterns).
    `misalign` passes fb_start 4 bytes off a 16-byte boundary."""
    from mrmt3 import lib
    so, t = lib.load(), c["t"]
    d = {k: torch.from_numpy(np.ascontiguousarray(t[k])).to(dev) for k in ("window", "twiddle", "fb_start", "fb_cnt", "fb_w")}
    audio = torch.from_numpy(c["audio"]).to(dev)
    vf = None if c["valid_frames"] is None else torch.from_numpy(c["valid_frames"]).to(dev)
    B = audio.shape[0] if c["seg_start"] is None else len(c["seg_start"])
    F = xl.n_frames_of(c["n_samples"], t["hop"])
    numel = B * F * t["n_mels"]
    buf = torch.full((GUARD + numel + GUARD,), SENTINEL, device=dev, dtype=torch.bfloat16 if bf16 else torch.float32)
    out = buf[GUARD:GUARD + numel]
    assert out.data_ptr() % 16 == 0 and d["fb_start"].data_ptr() % 16 == 0 and d["window"].data_ptr() % 8 == 0
    if misalign:
        d["fb_start"] = torch.cat([d["fb_start"][:1], d["fb_start"]])[1:]
        assert d["fb_start"].data_ptr() % 16 == 4
    before = lib.dispatch_counts()
    p, st = lib._p, lib._stream()
    if c["seg_start"] is None:
        rc = so.mrmt3_logmel_fwd(p(audio), B, c["n_samples"], t["hop"], p(d["window"]), p(d["twiddle"]), p(d["fb_start"]),
                                 p(d["fb_cnt"]), p(d["fb_w"]), t["n_mels"], t["max_taps"], p(vf), int(c["normalize"]), int(bf16),
                                 p(out), st)
    else:
        seg = torch.from_numpy(c["seg_start"]).to(dev)
        rc = so.mrmt3_logmel_crops_fwd(p(audio), audio.numel(), p(seg), B, c["n_samples"], t["hop"], p(d["window"]),
                                       p(d["twiddle"]), p(d["fb_start"]), p(d["fb_cnt"]), p(d["fb_w"]), t["n_mels"], t["max_taps"],
                                       p(vf), int(c["normalize"]), int(bf16), p(out), st)
    assert rc == 0, so.mrmt3_last_error()
    torch.cuda.synchronize()
    after = lib.dispatch_counts()
    took = {k: after[k] - before[k] for k in ("logmel_wave", "logmel_general")}
    assert took == {"logmel_wave": int(kernel == "wave"), "logmel_general": int(kernel == "general")}, (c["name"], kernel, took)
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + numel:] == SENTINEL).all()), c["name"] + ": wrote outside out"
    res = out.view(B, F, t["n_mels"]).cpu()
    return res.view(torch.int16).numpy().view(np.uint16) if bf16 else res.numpy()


def _run(c, dev, knobs, also_general=True, ref=None):
    """The case on the kernel its arguments select and, if that is the wave kernel, on the general one as well: bound on
    every element, floor rule, bf16 = RNE(f32).  Returns {kernel: observed ratio}."""
    ref = _ref(c) if ref is None else ref
    seen = {}
    for knob in (1, 0) if (c["kernel"] == "wave" and also_general) else (1,):
        knobs.set("MRMT3_LOGMEL", knob)
        kernel = xl.expected_kernel(c["t"], knob)
        got = _launch(c, dev, False, kernel)
        ratio, n_floor = xl.check(c["name"], got, ref, c, kernel)
        print("%s [%s]: ratio %.3f, floor-accepted %d" % (c["name"], kernel, ratio, n_floor))
        assert not c["noise"] or n_floor == 0
        if c.get("all_floor"):
            assert n_floor == got[:, :, c["t"]["fb_cnt"] > 0].size
        bits = _launch(c, dev, True, kernel)
        assert np.array_equal(bits, xl.bf16_rne_bits(got)), "%s [%s]: bf16 output is not RNE of the f32 output (%d differ)" % (
            c["name"], kernel, int((bits != xl.bf16_rne_bits(got)).sum()))
        seen[kernel] = ratio
    return seen


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(dev, knobs, name):
    """Sections A (every bin on its own), C (off the model's configuration), D (scaling edges) and E (crops and memory
    edges) of tests/_exact_logmel.py's `small_cases`."""
    c = CASES[name]
    if name in ("C_hop64", "C_hop256"):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        B, F = c["audio"].shape[0], xl.n_frames_of(c["n_samples"], c["t"]["hop"])
        assert xl.frames_per_workgroup(c["t"]["hop"], B, F, cus) > 8, "a wave of this case should walk more than one frame"
    _run(c, dev, knobs)
    if "k0s" in c:                                                   # closed form: bin k0 of frame 0 = 1024 A (2048 A at 0, 1024)
        knobs.set("MRMT3_LOGMEL", 1)
        got = _launch(c, dev, False, c["kernel"])
        first = int(c["t"]["fb_start"][0])
        for b, k0 in enumerate(c["k0s"]):
            if first <= k0 < first + c["t"]["n_mels"]:
                peak = (2048 if k0 in (0, 1024) else 1024) * xl.tone_amp(b, k0)
                assert abs(np.exp(float(got[b, 0, k0 - first])) - peak) <= (xl.K_of(c["kernel"]) * 2 + 16) * xl.U * peak * 2


def test_a_misaligned_table_is_seen_to_take_the_general_kernel(dev, knobs):
    """The wave kernel reads fb_start in 16-byte pieces; a table off that boundary goes to the general kernel, which the
    counters now show, and the result meets the general kernel's bound."""
    c = CASES["C_taps5"]
    knobs.set("MRMT3_LOGMEL", 1)
    assert c["kernel"] == "wave"
    got = _launch(c, dev, False, "general", misalign=True)
    xl.check(c["name"] + " (misaligned fb_start)", got, _ref(c), c, "general")


# ---- B. the frame counts production runs ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch64():
    c = xl.case("B_64", xl.coded_audio(64), xl.model_tables(), "wave", noise_case=True)
    return c, xl.reference(c)


@pytest.mark.parametrize("B", [16, 32, 64])
def test_production_batch(dev, knobs, batch64, B):
    """64 (32, 16) segments x 256 frames in one launch, the trainer's and the benchmark's shape: a wave walks 8 (4, 2)
    frames through its private LDS buffer.  All B x 256 x 512 elements against the reference, and bf16 = RNE(f32)."""
    c64, r64 = batch64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    fpw = xl.frames_per_workgroup(128, B, 256, cus)
    if cus == 256:
        assert fpw == B
    if B == 64:
        assert fpw > 8
    c = dict(c64, name="B_%d" % B, audio=c64["audio"][:B])
    ref = {k: (v if k == "W" else v[:B]) for k, v in r64.items()}
    _run(c, dev, knobs, also_general=(B == 64), ref=ref)


def test_production_batch_of_crops(dev, knobs):
    """The same shape through mrmt3_logmel_crops_fwd: 64 crops of one recording at odd sample offsets, valid_frames mixed
    (0 and 256 among them); what a crop must not see is NaN."""
    n, hop, B = 32768, 128, 64
    vf = np.array([(256, 0, 1, 100, 255, 256, 17, 64)[b % 8] for b in range(B)], np.int32)
    st = np.array([b * (n + 4096) + 2 * b + 1 for b in range(B)], np.int64)
    total = int(st[-1]) + n - 5000                                   # the last crop runs past the end of the recording
    rec = np.full(total, np.nan, np.float32)
    coded = xl.coded_audio(B, n, seed=5)
    for b in range(B):
        lim = min(n, total - int(st[b]), int(vf[b]) * hop)
        rec[st[b]:st[b] + lim] = coded[b, :lim]
    c = xl.case("B_crops", rec, xl.model_tables(), "wave", noise_case=True, seg_start=st, valid_frames=vf, n_samples=n)
    assert (st % 2 == 1).all() and xl.frames_per_workgroup(hop, B, 256, 256) == 64
    seen = _run(c, dev, knobs, also_general=False)
    assert set(seen) == {"wave"}
