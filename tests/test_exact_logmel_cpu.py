"""CPU companion of tests/test_exact_logmel_gpu.py: the fp64 reference of tests/_exact_logmel.py is right (direct DFT,
closed forms), its table constructions are valid inputs, a float32 restatement of the general kernel meets every bound
of every case with the chosen K and R, and every seeded fault is caught.  No GPU, no library."""
import math

import numpy as np
import pytest

import _exact_logmel as xl


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in xl.small_cases()}


@pytest.fixture(scope="module")
def refs(cases):
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = xl.reference(cases[name])
        return memo[name]
    return get


def test_reference_equals_a_direct_dft_and_the_closed_forms(cases, refs):
    # a direct O(N^2) DFT of a few frames, every bin on its own
    for name in ("A_noise_all", "A_offbin_all"):
        c = cases[name]
        xw = xl.frame_matrix(xl.rows_of(c), 128, 0, 17)[1, [0, 7, 16]] * c["t"]["window"].astype(np.float64)
        want = xl.dft_direct(xw)
        got = refs(name)["acc"][1, [0, 7, 16]]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(xw).sum(-1).max()
        assert np.allclose(refs(name)["L1"][1, [0, 7, 16]], np.abs(xw).sum(-1), rtol=1e-14)
    # an impulse: all 1025 bins equal window[n0 - f hop]; frames without it are silent
    win = xl.hann().astype(np.float64)
    r = refs("A_impulse_all")
    for b in range(2):
        n0 = 1000 + 301 * b
        for f in range(17):
            want = win[n0 - 128 * f] if 0 <= n0 - 128 * f < 2048 else 0.0
            assert np.abs(r["acc"][b, f] - want).max() <= 1e-12
            assert (r["out"][b, f] == (xl.LN_FLOOR if want == 0 else r["out"][b, f])).all()
    # on-bin cosines under a window of ones: bin k0 = 1024 A (2048 A at 0 and 1024), nothing elsewhere
    for i in range(0, len(xl.TONE_BINS), 2):
        k0s = xl.TONE_BINS[i:i + 2]
        c = cases["A_tone_%d_%d_all" % k0s]
        acc = xl.reference(c)["acc"]
        x64 = np.stack([xl.tone_amp(b, k0) * np.cos(2 * np.pi * ((k0 * np.arange(2048)) % 2048) / 2048) for b, k0 in enumerate(k0s)])
        exact = np.abs(np.fft.rfft(x64, axis=-1))                   # of the unrounded cosine
        for b, k0 in enumerate(k0s):
            A = xl.tone_amp(b, k0)
            peak = (2048 if k0 in (0, 1024) else 1024) * A
            assert abs(exact[b, k0] - peak) <= 1e-12 * peak
            assert abs(acc[b, 0, k0] - peak) <= 2048 * A * xl.U        # the f32 rounding of the samples, nothing more
            others = np.delete(acc[b, 0], k0)
            assert others.max() <= 2048 * A * xl.U
    # the two entry points differ past valid_frames * hop: the plain one only zeroes the frames
    c = dict(cases["D_clamps_raw"])
    plain = xl.reference(c)
    crop = dict(c, audio=c["audio"].reshape(-1), seg_start=np.arange(3) * c["n_samples"])
    cr = xl.reference(crop)
    assert (plain["out"][1, 3:] == 0).all() and (cr["out"][1, 3:] == 0).all()
    assert np.array_equal(plain["acc"][0], cr["acc"][0])
    assert not np.allclose(plain["acc"][1, 2], cr["acc"][1, 2])      # frame 2 of a 3-frame crop sees zeros from sample 384 on
    assert np.array_equal(plain["acc"][1, 0, :], plain["acc"][1, 0, :]) and (cr["L1"][1, 2] < plain["L1"][1, 2])
    # scaling: clamps, floor, normalisation
    n = xl.reference(cases["D_clamps"])
    assert n["out"].min() == 0.0 and n["out"].max() == 1.0
    live = n["live"][:, :, None] & np.ones_like(n["acc"], bool)
    assert (n["acc"][live] > math.exp(5)).any() and ((n["acc"][live] > 0) & (n["acc"][live] < math.exp(-12))).any()
    assert (n["out"][0] == 0).all() and n["live"][2].all()
    s = xl.reference(cases["D_silence_norm"])
    assert np.allclose(s["out"], (xl.LN_FLOOR + 12) / 17, rtol=0, atol=1e-15)


def test_table_constructions_are_valid_inputs(cases):
    for c in cases.values():
        xl.check_tables(c["t"], aligned_for_wave=c["kernel"] == "wave")
    lo, hi, al = xl.identity_tables(0, 512), xl.identity_tables(513, 512), xl.identity_tables(0, 1025)
    covered = set(lo["fb_start"]) | set(hi["fb_start"])
    assert covered == set(range(1025)) - {512} and set(al["fb_start"]) == set(range(1025))
    for taps in (1, 5, 12, 13, 40):
        t = xl.tri_tables(512, taps)
        assert t["fb_cnt"].max() == taps and t["fb_cnt"].min() == 1 and t["fb_start"][0] == 0
        assert (t["fb_start"] + t["fb_cnt"]).max() == 1025 and np.isnan(t["fb_w"]).any() == (taps > 1)
    h = xl.handmade_tables()
    assert [(int(h["fb_start"][m]), int(h["fb_cnt"][m])) for m in (0, 100, 200, 300)] == [(0, 3), (1020, 5), (1024, 1), (37, 0)]
    m = xl.model_tables()
    assert m["n_mels"] == 512 and m["max_taps"] <= 12 and (m["fb_cnt"] == 0).any()
    used = m["fb_cnt"] > 0                                           # (some of the lowest filters hold no bin at all)
    assert m["fb_start"][used].min() > 2 and (m["fb_start"] + m["fb_cnt"])[used].max() < 1000
    # the model's window is torch's periodic Hann, computed in f32: a few 2^-24 off the correctly rounded one, which is
    # why the reference takes the table that is passed as exact
    assert np.abs(m["window"].astype(np.float64) - xl.hann()).max() <= 2.0 ** -21
    # the launch's frames per workgroup on 256 CUs: the shapes section B and C mean to reach
    assert [xl.frames_per_workgroup(128, B, 256, 256) for B in (1, 12, 16, 32, 64)] == [8, 8, 16, 32, 64]
    assert xl.frames_per_workgroup(64, 4, 1025, 256) == 16 and xl.frames_per_workgroup(256, 4, 1025, 256) == 16
    assert [xl.frames_per_workgroup(h_, 2, 3, 256) for h_ in (8064, 8066)] == [2, 1] and xl.frames_per_workgroup(1000, 2, 6, 256) == 4
    # bf16 rounding helper against torch
    import torch
    x = np.concatenate([xl.noise(7, 1, 4096)[0], np.float32([1.00390625, 1.01171875, -1.00390625, 0.0, 1.0])])
    assert np.array_equal(xl.bf16_rne_bits(x), torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16))


def test_float32_restatement_meets_every_bound(cases, refs):
    worst = {}
    for name, c in cases.items():
        got = xl.restate_f32(c)
        ratio, n_floor = xl.check(name, got, refs(name), c, "general")
        worst[name] = ratio
        # the reference alone, rounded to f32, meets its own bound and the floor rule of the case
        _, ref_floor = xl.check(name + " (reference)", refs(name)["out"].astype(np.float32), refs(name), c, "wave")
        assert ref_floor <= n_floor and (ref_floor == 0 or c["allow_floor"])
        if c["noise"]:
            assert n_floor == 0
        if c.get("all_floor"):
            assert n_floor == got[:, :, c["t"]["fb_cnt"] > 0].size   # (an empty filter's floor is exact, not an acceptance)
    print("float32 restatement, observed ratios:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= min(xl.K_WAVE, xl.K_GENERAL)
    try:
        import scipy.fft as scipy_fft
    except ImportError:
        scipy_fft = None
    if scipy_fft is not None:                                        # second opinion: pocketfft in float32, bin by bin
        for name in ("A_noise_all", "A_offbin_all", "A_impulse_all", "A_tone_0_1_all", "A_tone_1023_1024_all"):
            c, r = cases[name], refs(name)
            xw = (xl.frame_matrix(xl.rows_of(c).astype(np.float32), 128, 0, 17).astype(np.float32) * c["t"]["window"])
            mag = np.abs(scipy_fft.rfft(xw, axis=-1))
            assert mag.dtype == np.float32
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(r["L1"][:, :, None] > 0, np.abs(mag - r["acc"]) / (xl.U * r["L1"][:, :, None]), 0.0)
            assert q.max() <= min(xl.K_WAVE, xl.K_GENERAL), (name, q.max())


def _big_case():
    t = xl.model_tables()
    return xl.case("B_64", xl.coded_audio(64), t, "wave", noise_case=True)


@pytest.fixture(scope="module")
def big():
    c = _big_case()
    return c, xl.reference(c)


def test_production_batch_reference_and_restatement(big):
    c, r = big
    assert r["acc"].shape == (64, 256, 512) and (r["acc"] > 0)[:, :, c["t"]["fb_cnt"] > 0].all()
    # every frame its own: no two frames of the batch (nor a frame and the one 8 after it) within 1 % in more than a few bins
    lg = np.log(np.where(r["acc"] > 0, r["acc"], 1.0))
    d8 = np.abs(lg[:, 8:] - lg[:, :-8])[:, :, c["t"]["fb_cnt"] > 0]
    assert (np.median(d8, axis=-1) > 0.05).all()
    got = xl.restate_f32(dict(c, audio=c["audio"][:4]))
    sub = {k: (v[:4] if k != "W" else v) for k, v in r.items()}
    ratio, n_floor = xl.check("B_4of64", got, sub, c, "general")
    assert n_floor == 0
    # one element of the whole batch off by 4x its bound is caught, and named
    full = np.where(r["acc"] > 0, lg, xl.LN_FLOOR).astype(np.float32)
    xl.check("B_64 rounded reference", full, r, c, "wave")
    b, f, m = 41, 203, 377
    K = xl.K_WAVE
    bound = K * xl.U * r["L1"][b, f] * r["W"][m] + ((c["t"]["fb_cnt"][m] + 4) * xl.U + 4 * xl.U * abs(lg[b, f, m])) * r["acc"][b, f, m]
    full[b, f, m] = np.float32(math.log(r["acc"][b, f, m] + 4 * bound))
    with pytest.raises(AssertionError, match=r"row 41, frame 203, mel 377"):
        xl.check("B_64 one element", full, r, c, "wave")


FAULTS = [  # (fault, the case that must catch it)
    ("twiddle_index", "A_noise_all"), ("twiddle_index", "C_hop126"),
    ("window_shift", "A_noise_lo"), ("window_shift", "C_taps12"),
    ("hann_symmetric", "A_offbin_all"), ("hann_symmetric", "C_hop126"),
    ("swap_bins", "A_offbin_all"), ("swap_bins", "A_tone_2_15_all"), ("swap_bins", "C_taps5"),
    ("nyquist_from_dc", "A_tone_0_1_all"), ("nyquist_from_dc", "A_noise_hi"), ("nyquist_from_dc", "C_handmade"),
    ("nyquist_dropped", "A_tone_1023_1024_all"), ("nyquist_dropped", "A_noise_hi"), ("nyquist_dropped", "C_handmade"),
    ("frame_plus_8", "A_noise_lo"), ("frame_plus_8", "C_hop126"),
    ("tap_leak", "C_taps5"), ("tap_leak", "C_handmade"), ("tap_leak", "C_taps13"),
    ("no_clamp", "D_clamps"),
    ("sqrt_approx", "A_tone_0_1_all"), ("sqrt_approx", "A_tone_511_512_all"),
]


@pytest.mark.parametrize("fault,name", FAULTS)
def test_seeded_fault_is_caught(cases, refs, fault, name):
    c = cases[name]
    good = xl.restate_f32(c)
    bad = xl.restate_f32(c, fault=fault)
    assert not np.array_equal(good, bad), "the fault changes nothing in this case"
    with pytest.raises(AssertionError):
        xl.check(name, bad, refs(name), c, "general")


def test_frame_fault_is_caught_in_the_production_batch(big):
    c, r = big
    sub_case = dict(c, audio=c["audio"][:2])
    sub = {k: (v[:2] if k != "W" else v) for k, v in r.items()}
    with pytest.raises(AssertionError):
        xl.check("B frame + 8", xl.restate_f32(sub_case, fault="frame_plus_8"), sub, c, "wave")


def test_bf16_truncation_is_caught(cases):
    v = xl.restate_f32(cases["D_clamps"])
    want, trunc = xl.bf16_rne_bits(v), xl.bf16_trunc_bits(v)
    inner = (v != 0) & (v != 1)
    assert (want != trunc)[inner].mean() > 0.4                             # truncation differs wherever the dropped bits round up
    x = np.float32([1.00390625, 1.01171875, np.nextafter(np.float32(1.00390625), np.float32(2)), 3.0])         # ties to even (down, up), just above a tie, exact
    assert xl.bf16_rne_bits(x).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x4040]
