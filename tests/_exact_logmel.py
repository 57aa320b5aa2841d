"""Constructions, the fp64 reference, bounds and checkers of the per-bin tests of the log-mel kernels of csrc/logmel.hip
(tests/test_exact_logmel_gpu.py; proven on the CPU by tests/test_exact_logmel_cpu.py).  numpy only; nothing here touches
the library.

Reference (`reference`): the contract of include/mrmt3_hip.h restated, not the kernels.  Frame f of a row is samples
[f hop, f hop + 2048), zero past n_samples (crops: also past the end of the recording and past valid_frames * hop; the
plain entry point only zeroes the FRAMES >= valid_frames), times the f32 window table taken as exact, |np.fft.rfft| in
float64, acc[m] = sum_{q < fb_cnt[m]} fb_w[m, q] mag[fb_start[m] + q] in float64 on the f32 table values, ln(acc) with
ln 1e-5 where acc <= 0, clamp to [-12, 5] and (v + 12) / 17 when normalising, zeros for frames >= valid_frames.

Bound (`check`), linear domain, EVERY element:   |exp(got) - acc| <= K u L1_f W_m + R_m acc,   u = 2^-24,
  L1_f = sum_n |x_n w_n| of the frame (a cap on every |X[k]| and the scale of the transform's rounding),
  W_m  = sum_{q < cnt} |fb_w[m, q]|,
  R_m  = (cnt_m + 4) u + 4 u |ln acc|: relative error of everything behind the transform, first order --
         |X|^2 = fl(fl(x^2) + fl(y^2)) errs by 2 u, its root by half of that, u; v_sqrt_f32 is good to one ulp = 2 u;
         tap q costs one product and (but the first) one addition, cnt u in all on non-negative terms (every table here
         is non-negative, asserted); v_log_f32 at one ulp of log2 acc, the f32 constant ln 2 and the product by it move
         ln acc by (2 + 1 + 1) u |ln acc|, which is that relative error of exp(got); one more u for second-order terms
         and the f32 result.  The general kernel's logf is no worse.
  Normalised output: got 17 - 12 is held to the same bound with 3 * 17 u more relative error (the subtraction and the
  division each round a value of at most 17; one u to spare), and the clamps are exact: acc clearly above e^5 must give
  1.0, acc clearly inside (0, e^-12) must give 0.0, bit for bit.
  Floor rule: an element that misses the bound but equals the floor value ln 1e-5 is accepted iff acc <= K u L1_f W_m (a
  computed zero where the exact value is below the kernel's resolution); `check` returns how many were, and every noise
  case demands zero.
  bf16 output: round-to-nearest-even of the f32 output of the same call and kernel, bit for bit (`bf16_rne_bits`).

K: 3x the largest observed ratio (|exp(got) - acc| - R acc) / (u L1 W) over every case on an MI355X, per kernel:
  K_WAVE = 3 x 1.438 = 4.32, K_GENERAL = 3 x 1.514 = 4.55.  Both maxima are on-bin cosines under the window of ones, the
  one input whose spectrum is as large as L1 allows; the a-priori ceiling (eleven radix-2 levels at a few roundings each)
  is about 40, and a ratio above K_FINDING = 16 would be a finding to explain, not a tolerance.  For scale: pocketfft in
  float32 stays between 0.2 and 3.5 on the same kinds of input, the float32 restatement of the general kernel below 1.06.
  Observed per group of cases (largest element; `pytest -s` prints every case):         wave    general
    A  noise, identity filters (bins 0-511, 513-1024 / all 1025)                          0.223   0.208
    A  impulse per row                                                                    0       0
    A  on-bin cosines, window of ones, 16 bins                                            1.438   1.514
    A  Hann-windowed tone between bins + partial 80 dB down                               0.841   0.806
    B  16 / 32 / 64 segments x 256 frames (fpw 16 / 32 / 64), 64 crops                    0.478   0.416 (64 only)
    C  hop 2 / 64 / 126 / 256 / 1000 / 8064 / 8066                                        0.438   0.323
    C  hop 125, n_mels 1 / 128 / 229, max_taps 13 / 40                                    -       0.182
    C  max_taps 1 / 5 / 12, hand-made filters, n_samples 1 / 127 / 2048 / 2049            0.353   0.214
    D  clamps, silence                                                                    0.050   0.096
    E  crops at the edges of a NaN-filled recording                                       0.140   0.196
  The bf16 output equalled RNE of the f32 output bit for bit in every case on both kernels.
"""
import math

import numpy as np

U = 2.0 ** -24
FFT_N, NB = 2048, 1025
LN_FLOOR = math.log(1e-5)
FLOOR32 = float(np.log(np.float32(1e-5)))          # what both kernels store for acc <= 0
LO, HI = -12.0, 5.0
NORM_EXTRA = 3 * 17 * U
K_WAVE = 4.32                                      # 3 x 1.438, see above
K_GENERAL = 4.55                                   # 3 x 1.514
K_FINDING = 16.0                                   # an observed ratio above this is a finding to explain
assert max(K_WAVE, K_GENERAL) <= K_FINDING


def K_of(kernel):
    return K_WAVE if kernel == "wave" else K_GENERAL


# ---- tables -------------------------------------------------------------------------------------------------------------------

def hann(periodic=True):
    n = np.arange(FFT_N, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2 * np.pi * n / (FFT_N if periodic else FFT_N - 1))).astype(np.float32)


def twiddle_table():
    k = np.arange(FFT_N // 2, dtype=np.float64)
    return np.stack([np.cos(-2 * np.pi * k / FFT_N), np.sin(-2 * np.pi * k / FFT_N)], axis=1).astype(np.float32)


def tables(start, cnt, w, hop=128, window=None):
    start, cnt, w = np.asarray(start, np.int32), np.asarray(cnt, np.int32), np.asarray(w, np.float32)
    return dict(hop=hop, n_mels=len(start), max_taps=w.shape[1], fb_start=start, fb_cnt=cnt, fb_w=np.ascontiguousarray(w),
                window=hann() if window is None else np.asarray(window, np.float32), twiddle=twiddle_table())


def model_tables(hop=128):
    """The model's own tables (contrib.spectrograms.kernel_tables: 512 HTK filters over 20-7600 Hz, periodic Hann)."""
    import torch
    from contrib import spectrograms as sp
    t = sp.kernel_tables(sp.SpectrogramConfig(), torch.device("cpu"))        # (cached there per device)
    return dict(hop=hop, n_mels=t["n_mels"], max_taps=t["max_taps"], fb_start=t["fb_start"].numpy().copy(),
                fb_cnt=t["fb_cnt"].numpy().copy(), fb_w=t["fb_w"].numpy().copy(), window=t["window"].numpy().copy(),
                twiddle=t["twiddle"].numpy().copy())


def identity_tables(first, n_mels, window=None):
    """Filter m = bin first + m alone, weight 1: every bin on its own."""
    return tables(first + np.arange(n_mels), np.ones(n_mels), np.ones((n_mels, 1)), window=window)


def tri_tables(n_mels, max_taps, hop=128, scale=None, nan_tail=True):
    """Triangular filters of 1 .. max_taps taps whose starts sweep bins 0 .. 1025 - cnt (first filter at bin 0, last one
    ending on bin 1024), filter 0 the widest; NaN behind every filter's last tap."""
    m = np.arange(n_mels)
    cnt = 1 + (m * 11 + max_taps - 1) % max_taps
    start = np.round(m * (NB - cnt) / max(n_mels - 1, 1)).astype(np.int64) if n_mels > 1 else np.array([NB - max_taps])
    q = np.arange(max_taps)[None, :]
    w = 1.0 - np.abs((q + 0.5) / cnt[:, None] * 2 - 1) * 0.9
    if scale is not None:
        w = w * np.asarray(scale, np.float64)[:, None]
    w = np.where(q < cnt[:, None], w, np.nan if nan_tail else 0.0)
    return tables(start, cnt, w, hop=hop)


def handmade_tables():
    """512 filters for the wave kernel, most of them the model's shape in miniature, five made by hand: bins 0-2, bins
    1020-1024, the Nyquist bin alone, an empty filter (the floor), and NaN behind every count."""
    t = tri_tables(512, 5)
    for m, (s, c) in {0: (0, 3), 100: (1020, 5), 200: (1024, 1), 300: (37, 0), 511: (1022, 3)}.items():
        t["fb_start"][m], t["fb_cnt"][m] = s, c
        t["fb_w"][m] = np.where(np.arange(5) < c, 0.25 + 0.5 * np.arange(5), np.nan)
    return t


def check_tables(t, aligned_for_wave):
    """The table is a valid input of the contract (and, when meant for the wave kernel, has its shape)."""
    s, c, w = t["fb_start"].astype(np.int64), t["fb_cnt"].astype(np.int64), t["fb_w"]
    assert s.shape == c.shape == (t["n_mels"],) and w.shape == (t["n_mels"], t["max_taps"]) and w.dtype == np.float32
    assert (s >= 0).all() and (s <= 1024).all() and (c >= 0).all() and (c <= t["max_taps"]).all() and (s + c <= NB).all()
    live = np.arange(t["max_taps"])[None, :] < c[:, None]
    assert np.isfinite(w[live]).all() and (w[live] >= 0).all(), "the bound's R term assumes non-negative taps"
    assert t["window"].shape == (FFT_N,) and t["window"].dtype == np.float32 and t["twiddle"].shape == (1024, 2)
    assert expected_kernel(t) == ("wave" if aligned_for_wave else "general")


def expected_kernel(t, knob=1):
    """include/mrmt3_hip.h: the wave kernel takes n_mels = 512, max_taps <= 12 and an even hop (tables aligned, which every
    fresh allocation is); the general kernel everything else, and everything under MRMT3_LOGMEL=0."""
    return "wave" if knob and t["n_mels"] == 512 and t["max_taps"] <= 12 and t["hop"] % 2 == 0 and t["hop"] >= 2 else "general"


def frames_per_workgroup(hop, batch, n_frames, cus):
    """logmel_launch's choice for the wave kernel: as many frames as the 10112-float strip holds, at most 64, halved while
    above 8 until the grid covers the CUs."""
    fpw = min((10112 - FFT_N) // hop + 1, 64)
    while fpw > 8 and (batch * n_frames) // fpw < cus:
        fpw >>= 1
    return min(fpw, n_frames)


# ---- the fp64 reference -------------------------------------------------------------------------------------------------------

def n_frames_of(n_samples, hop):
    return -(-n_samples // hop)


def rows_of(case):
    """[B, n_samples] float64: what each row of the call may see, zeros elsewhere."""
    a, n = case["audio"], case["n_samples"]
    if case.get("seg_start") is None:
        return np.asarray(a, np.float64).reshape(-1, n)
    hop, vf = case["t"]["hop"], case.get("valid_frames")
    rows = np.zeros((len(case["seg_start"]), n))
    for b, st in enumerate(case["seg_start"]):
        lim = min(n, len(a) - int(st))
        if vf is not None:
            lim = min(lim, int(vf[b]) * hop)
        if lim > 0:
            rows[b, :lim] = a[int(st):int(st) + lim]
    return rows


def mel_sums(mag, t):
    """acc [.., M] = sum_{q < cnt} fb_w[m, q] mag[.., start + q] in float64 (what lies behind a count is never read), and
    W [M] = sum_{q < cnt} |fb_w[m, q]|."""
    s, c = t["fb_start"].astype(np.int64), t["fb_cnt"].astype(np.int64)
    acc, W = np.zeros(mag.shape[:-1] + (t["n_mels"],)), np.zeros(t["n_mels"])
    for q in range(t["max_taps"]):
        m = np.nonzero(q < c)[0]
        w = t["fb_w"][m, q].astype(np.float64)
        acc[..., m] += mag[..., s[m] + q] * w
        W[m] += np.abs(w)
    return acc, W


def frame_matrix(rows, hop, f0, f1):
    """[B, f1 - f0, 2048] float64 frames of zero-padded rows."""
    B, n = rows.shape
    idx = (np.arange(f0, f1) * hop)[:, None] + np.arange(FFT_N)[None, :]
    pad = np.concatenate([rows, np.zeros((B, 1))], axis=1)
    return pad[:, np.minimum(idx, n)]


def reference(case, chunk=4096):
    """dict(acc [B, F, M], L1 [B, F], W [M], live [B, F] bool (frames < valid_frames), out [B, F, M]) in float64."""
    t, rows = case["t"], rows_of(case)
    B, F = rows.shape[0], n_frames_of(case["n_samples"], t["hop"])
    win = t["window"].astype(np.float64)
    acc, L1 = np.empty((B, F, t["n_mels"])), np.empty((B, F))
    per = max(1, chunk // B)
    for f0 in range(0, F, per):
        f1 = min(F, f0 + per)
        xw = frame_matrix(rows, t["hop"], f0, f1) * win
        L1[:, f0:f1] = np.abs(xw).sum(-1)
        acc[:, f0:f1], W = mel_sums(np.abs(np.fft.rfft(xw, axis=-1)), t)
    vf = case.get("valid_frames")
    live = np.ones((B, F), bool) if vf is None else np.arange(F)[None, :] < np.asarray(vf)[:, None]
    with np.errstate(divide="ignore"):
        out = np.where(acc > 0, np.log(np.where(acc > 0, acc, 1.0)), LN_FLOOR)
    if case.get("normalize"):
        out = (np.clip(out, LO, HI) - LO) / (HI - LO)
    out = np.where(live[:, :, None], out, 0.0)
    return dict(acc=acc, L1=L1, W=W, live=live, out=out)


def dft_direct(xw):
    """O(N^2) one-sided DFT magnitudes of a few windowed frames [F, 2048], float64 (longdouble phases)."""
    n = np.arange(FFT_N, dtype=np.int64)
    k = np.arange(NB, dtype=np.int64)[:, None]
    ph = ((k * n) % FFT_N).astype(np.longdouble) * (2 * np.pi / np.longdouble(FFT_N))
    c, s = np.cos(ph).astype(np.float64), np.sin(ph).astype(np.float64)
    return np.hypot(xw @ c.T, xw @ s.T)


# ---- checkers -----------------------------------------------------------------------------------------------------------------

def check(name, got, ref, case, kernel, K=None, allow_floor=None):
    """Every element of `got` (float32 [B, F, M]) against `ref`.  Returns (observed ratio, floor-accepted count); raises
    naming the worst element."""
    K = K_of(kernel) if K is None else K
    t = case["t"]
    acc, L1, W, live = ref["acc"], ref["L1"], ref["W"], ref["live"]
    assert got.shape == acc.shape and got.dtype == np.float32, (name, got.shape, got.dtype, acc.shape)
    assert np.isfinite(got).all(), name + ": output not finite"
    g = got.astype(np.float64)
    dead = ~live
    assert (got[dead] == 0).all(), name + ": a frame >= valid_frames is not zero"
    scale = U * L1[:, :, None] * W[None, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        lnacc = np.where(acc > 0, np.abs(np.log(np.where(acc > 0, acc, 1.0))), 0.0)
    R = (t["fb_cnt"].astype(np.float64)[None, None, :] + 4) * U + 4 * U * lnacc
    floor_val = FLOOR32
    if case.get("normalize"):
        R = R + NORM_EXTRA
        floor_val = float((np.float32(FLOOR32) - np.float32(LO)) / np.float32(HI - LO))
        one, zero = g == 1.0, g == 0.0
        lin = np.exp(g * (HI - LO) + LO)
        # exact clamps: clearly above e^5 -> 1.0, clearly inside (0, e^-12) -> 0.0
        hi_sure = live[:, :, None] & (acc * (1 - 1e-3) - K * scale > math.exp(HI))
        lo_sure = live[:, :, None] & (acc > 0) & (acc * (1 + 1e-3) + K * scale < math.exp(LO))
        assert one[hi_sure].all(), "%s: %d elements above e^5 are not exactly 1.0" % (name, int((~one[hi_sure]).sum()))
        assert zero[lo_sure].all(), "%s: %d elements inside (0, e^-12) are not exactly 0.0" % (name, int((~zero[lo_sure]).sum()))
    else:
        lin = np.exp(g)
    err = np.abs(lin - acc)
    if case.get("normalize"):          # a clamped output stands for everything beyond the clamp
        err = np.where(one, np.maximum(math.exp(HI) - acc, 0.0), err)
        err = np.where(zero, np.maximum(acc - math.exp(LO), 0.0), err)
    excess = np.maximum(err - R * acc, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(excess == 0, 0.0, excess / scale)
    ratio = np.where(live[:, :, None], ratio, 0.0)
    at_floor = np.abs(g - floor_val) <= 4 * U * abs(floor_val) + (NORM_EXTRA if case.get("normalize") else 0.0)
    empty = live[:, :, None] & (t["fb_cnt"] == 0)[None, None, :]       # a filter without taps: the floor is the exact answer
    assert at_floor[empty].all(), name + ": an empty filter does not give ln 1e-5"
    ratio = np.where(empty, 0.0, ratio)
    floored = live[:, :, None] & (ratio > K) & at_floor & (acc <= K * scale)
    n_floor = int(floored.sum())
    ratio = np.where(floored, 0.0, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= K:
        b, f, m = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError("%s [%s]: ratio %.4g > K %.4g at (row %d, frame %d, mel %d): got %.9g, want ln acc = %.9g (acc %.6g, "
                             "L1 %.6g, W %.6g); %d of %d elements out" % (name, kernel, worst, K, b, f, m, g[b, f, m],
                                                                          math.log(acc[b, f, m]) if acc[b, f, m] > 0 else LN_FLOOR,
                                                                          acc[b, f, m], L1[b, f], W[m], int((ratio > K).sum()), ratio.size))
    allow = case.get("allow_floor", False) if allow_floor is None else allow_floor
    assert allow or n_floor == 0, "%s [%s]: %d elements accepted by the floor rule in a case that allows none" % (name, kernel, n_floor)
    return worst, n_floor


def bf16_rne_bits(x):
    """uint16 bfloat16 bit patterns of float32 `x`, round to nearest even (finite values)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_trunc_bits(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


# ---- inputs -------------------------------------------------------------------------------------------------------------------

N_A = 16 * 128 + 5
TONE_BINS = (0, 1, 2, 15, 16, 17, 63, 64, 255, 256, 511, 512, 513, 767, 1023, 1024)


def noise(seed, B, n, amp=1.0):
    return (np.random.RandomState(seed).uniform(-1, 1, size=(B, n)) * amp).astype(np.float32)


def impulses(B, n):
    """one unit impulse per row: frame f sees it at sample n0 - f hop, a different place in every frame that holds it"""
    x = np.zeros((B, n), np.float32)
    for b in range(B):
        x[b, 1000 + 301 * b] = 1.0
    return x


def on_bin_tones(k0s, n):
    """row b: A_b cos(2 pi k0_b n / 2048) -- with a window of ones bin k0 is 1024 A (2048 A for k0 = 0, 1024)"""
    i = np.arange(n, dtype=np.int64)
    return np.stack([(0.75 ** b / 1024.0 * (1 + k0 % 3)) * np.cos(2 * np.pi * ((k0 * i) % FFT_N) / FFT_N)
                     for b, k0 in enumerate(k0s)]).astype(np.float32)


def tone_amp(b, k0):
    return 0.75 ** b / 1024.0 * (1 + k0 % 3)


def off_bin_tone(B, n):
    i = np.arange(n, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * (100.37 + 211 * b) * i / FFT_N + b) + 1e-4 * np.cos(2 * np.pi * (700.5 - 90 * b) * i / FFT_N)
                     for b in range(B)]).astype(np.float32)


def coded_audio(B, n=32768, hop=128, seed=3):
    """Noise plus a tone per 128-sample block, both scaled by a non-monotone code of (row, block): no two frames of the
    batch alike, neighbours a power of two apart, rows offset against each other."""
    rs = np.random.RandomState(seed)
    blk = np.arange(n) // hop
    i = np.arange(n, dtype=np.float64)
    x = np.empty((B, n), np.float32)
    for b in range(B):
        amp = 2.0 ** (((b * 37 + blk * 11) % 13) - 8.0)
        f = 3 + (b * 29 + blk * 53) % 900
        x[b] = amp * (rs.uniform(-1, 1, n) + np.cos(2 * np.pi * f * i / FFT_N))
    return x


def case(name, audio, t, kernel=None, noise_case=False, allow_floor=False, **kw):
    audio = np.ascontiguousarray(audio, np.float32)
    c = dict(name=name, audio=audio, t=t, noise=noise_case, allow_floor=allow_floor, valid_frames=None, normalize=False,
             seg_start=None)
    c.update(kw)
    if c["seg_start"] is None:
        c["n_samples"] = audio.shape[1]
    if c["valid_frames"] is not None:
        c["valid_frames"] = np.asarray(c["valid_frames"], np.int32)
    if c["seg_start"] is not None:
        c["seg_start"] = np.asarray(c["seg_start"], np.int64)
    c["kernel"] = expected_kernel(t)
    assert kernel is None or kernel == c["kernel"], (name, kernel, c["kernel"])
    return c


def crop_recording(total, seg_start, n_samples, hop, valid_frames, seed):
    """A recording that is NaN wherever the contract says no crop may look: only [st, st + lim) of each crop holds samples."""
    rs = np.random.RandomState(seed)
    a = np.full(total, np.nan, np.float32)
    for b, st in enumerate(seg_start):
        lim = min(n_samples, total - st, int(valid_frames[b]) * hop)
        if lim > 0:
            assert np.isnan(a[st:st + lim]).all(), "crops overlap"
            a[st:st + lim] = rs.uniform(-1, 1, lim) * 2.0 ** -(b % 5)
    return a


def small_cases():
    """Every case of sections A, C, D and E: a list of dicts (see `case`).  Section B's batches are built by the tests."""
    out = []
    ones = np.ones(FFT_N, np.float32)
    idt = {"lo": lambda w=None: identity_tables(0, 512, w), "hi": lambda w=None: identity_tables(513, 512, w),
           "all": lambda w=None: identity_tables(0, 1025, w)}
    # A. every bin on its own
    for tn, mk in idt.items():
        kern = "general" if tn == "all" else "wave"
        out.append(case("A_noise_" + tn, noise(1, 2, N_A), mk(), kern, noise_case=True))
        out.append(case("A_impulse_" + tn, impulses(2, N_A), mk(), kern, allow_floor=True))
        out.append(case("A_offbin_" + tn, off_bin_tone(2, N_A), mk(), kern))
        for i in range(0, len(TONE_BINS), 2):
            k0s = TONE_BINS[i:i + 2]
            out.append(case("A_tone_%d_%d_%s" % (k0s + (tn,)), on_bin_tones(k0s, N_A), mk(ones), kern, allow_floor=True, k0s=k0s))
    # C. off the model's configuration
    mt = model_tables
    for hop, B, n in ((2, 2, 300), (64, 4, 64 * 1024 + 3), (126, 2, 126 * 9 + 60), (256, 4, 256 * 1024 + 3), (1000, 2, 5007),
                      (8064, 2, 8064 * 2 + 100), (8066, 2, 8066 * 2 + 100), (125, 2, 125 * 9 + 60)):
        out.append(case("C_hop%d" % hop, noise(20 + hop % 7, B, n, 0.5), mt(hop), "general" if hop == 125 else "wave", noise_case=True))
    for n_mels in (1, 128, 229):
        out.append(case("C_mels%d" % n_mels, noise(31, 2, N_A), tri_tables(n_mels, 9), "general", noise_case=True))
    for taps in (13, 40):
        out.append(case("C_taps%d" % taps, noise(32, 2, N_A), tri_tables(512, taps), "general", noise_case=True))
    for taps in (1, 5, 12):
        out.append(case("C_taps%d" % taps, noise(33, 2, N_A), tri_tables(512, taps), "wave", noise_case=True))
    out.append(case("C_handmade", noise(34, 2, N_A), handmade_tables(), "wave", allow_floor=True))
    for n in (1, 127, 2048, 2049):
        # (n = 1 and the last frame of n = 2049 hold sample 0 of the window alone, which is 0: silent frames, the floor)
        out.append(case("C_n%d" % n, noise(35, 2, n) + np.float32(0.25), mt(), "wave", noise_case=n in (127, 2048),
                        allow_floor=n in (1, 2049)))
    # D. scaling edges: filters of weight 1e3, 1 and 1e-8 in turn put mel bins above e^5, in between and inside (0, e^-12)
    sc = np.array([1e3, 1.0, 1e-8])[np.arange(512) % 3]
    F = n_frames_of(N_A, 128)
    out.append(case("D_clamps", noise(41, 3, N_A), tri_tables(512, 7, scale=sc), "wave", noise_case=True, normalize=True,
                    valid_frames=[0, F, F + 5]))
    out.append(case("D_clamps_raw", noise(41, 3, N_A), tri_tables(512, 7, scale=sc), "wave", noise_case=True,
                    valid_frames=[F + 5, 3, 0]))
    out.append(case("D_silence", np.zeros((2, N_A)), mt(), "wave", allow_floor=True, all_floor=True))
    out.append(case("D_silence_norm", np.zeros((2, N_A)), mt(), "wave", allow_floor=True, all_floor=True, normalize=True))
    # E. crops and memory edges
    n, hop, total = 16 * 128, 128, 30000
    vf = [16, 16, 7, 0, 16]
    for tag, last in (("end", total - 1500), ("last", total - 1)):   # (the two overlap: one recording each)
        st = [0, 4001, 9000 + 777, 16001, last]
        for norm in (False, True):
            out.append(case("E_crops_" + tag + ("_norm" if norm else ""), crop_recording(total, st, n, hop, vf, 51), mt(), "wave",
                            allow_floor=True, seg_start=st, valid_frames=vf, n_samples=n, normalize=norm))
        out.append(case("E_crops_general_" + tag, crop_recording(total, st, n, hop, vf, 53), tri_tables(229, 9), "general",
                        allow_floor=True, seg_start=st, valid_frames=vf, n_samples=n))
    out.append(case("E_short_recording", crop_recording(1500, [0], n, hop, [16], 52), mt(), "wave", allow_floor=True,
                    seg_start=[0], valid_frames=[16], n_samples=n))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


# ---- the general kernel restated in float32 (the CPU companion's stand-in for the device; carries the seeded faults) -----

def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def restate_f32(case, fault=None):
    """csrc/logmel.hip's workgroup-per-frame kernel operation by operation on float32 arrays, all frames at once: packed
    1024-point radix-4 Stockham transform, real-input unpack, magnitudes, mel sums in tap order, log, clamp and scale.
    `fault` seeds one defect (tests/test_exact_logmel_cpu.py lists them).  Returns float32 [B, F, M]."""
    f32 = np.float32
    t = case["t"]
    hop, M, T = t["hop"], t["n_mels"], t["max_taps"]
    rows = rows_of(case).astype(f32)
    B, n = rows.shape
    F = n_frames_of(n, hop)
    win = t["window"]
    if fault == "window_shift":
        win = np.concatenate([win[1:], win[:1]])
    if fault == "hann_symmetric":
        win = hann(periodic=False)
    fr = frame_matrix(rows, hop, 0, F).astype(f32)
    if fault == "frame_plus_8":
        fr = np.concatenate([fr[:, 8:], fr[:, :8]], axis=1)
    xw = (fr * win).reshape(B * F, FFT_N)
    re, im = xw[:, 0::2].copy(), xw[:, 1::2].copy()
    tw = t["twiddle"]

    def twid(idx):
        sgn = np.where(idx & 1024, f32(-1), f32(1))
        return tw[idx & 1023, 0] * sgn, tw[idx & 1023, 1] * sgn

    tid = np.arange(256)
    for p_ in range(5):
        p = 1 << (2 * p_)
        k = tid & (p - 1)
        j = ((tid - k) << 2) + k
        twm = (512 >> (2 * p_)) * k
        if fault == "twiddle_index" and p_ == 3:
            twm = twm + 1
        u0r, u0i = re[:, tid], im[:, tid]
        u1r, u1i = _cmul(re[:, tid + 256], im[:, tid + 256], *twid(twm))
        u2r, u2i = _cmul(re[:, tid + 512], im[:, tid + 512], *twid(2 * twm))
        u3r, u3i = _cmul(re[:, tid + 768], im[:, tid + 768], *twid(3 * twm))
        v0r, v0i, v1r, v1i = u0r + u2r, u0i + u2i, u0r - u2r, u0i - u2i
        v2r, v2i = u1r + u3r, u1i + u3i
        dr, di = u1r - u3r, u1i - u3i
        v3r, v3i = di, -dr
        nre, nim = np.empty_like(re), np.empty_like(im)
        nre[:, j], nim[:, j] = v0r + v2r, v0i + v2i
        nre[:, j + p], nim[:, j + p] = v1r + v3r, v1i + v3i
        nre[:, j + 2 * p], nim[:, j + 2 * p] = v0r - v2r, v0i - v2i
        nre[:, j + 3 * p], nim[:, j + 3 * p] = v1r - v3r, v1i - v3i
        re, im = nre, nim
    k = np.arange(NB)
    zkr, zki = re[:, k & 1023], im[:, k & 1023]
    znr, zni = re[:, (1024 - k) & 1023], im[:, (1024 - k) & 1023]
    h = f32(0.5)
    ar, ai, br, bi = h * (zkr + znr), h * (zki - zni), h * (zkr - znr), h * (zki + zni)
    wr = np.concatenate([tw[:, 0], [f32(-1)]]).astype(f32)
    wi = np.concatenate([tw[:, 1], [f32(0)]]).astype(f32)
    wbr, wbi = _cmul(wr, wi, br, bi)
    Xr, Xi = ar + wbi, ai - wbr
    mag = np.sqrt(Xr * Xr + Xi * Xi)
    if fault == "swap_bins":
        mag = mag[:, ::-1].copy()
        mag[:, [0, 1024]] = mag[:, [1024, 0]]                       # bins k and 1024 - k exchanged, 0 and 1024 kept
    if fault == "nyquist_from_dc":
        mag[:, 1024] = mag[:, 0]
    if fault == "nyquist_dropped":
        mag[:, 1024] = 0
    if fault == "sqrt_approx":
        mag = mag * f32(1 + 2e-6)
    s, c = t["fb_start"].astype(np.int64), t["fb_cnt"].astype(np.int64)
    if fault == "tap_leak":
        c = np.minimum(c + 1, T)
    acc = np.zeros((B * F, M), f32)
    magp = np.concatenate([mag, np.zeros((B * F, T), f32)], axis=1)
    for q in range(T):
        on = q < c
        w = np.where(on, np.where(np.isnan(t["fb_w"][:, q]) & on, f32(1e30), t["fb_w"][:, q]), f32(0)).astype(f32)
        acc = acc + magp[:, s + q] * w
    v = np.log(np.where(acc <= 0, f32(1e-5), acc)).astype(f32)
    if case.get("normalize"):
        if fault != "no_clamp":
            v = np.minimum(np.maximum(v, f32(LO)), f32(HI))
        v = ((v - f32(LO)) / f32(HI - LO)).astype(f32)
    v = v.reshape(B, F, M)
    vf = case.get("valid_frames")
    if vf is not None:
        v = np.where((np.arange(F)[None, :] < np.asarray(vf)[:, None])[:, :, None], v, f32(0))
    return np.ascontiguousarray(v, f32)
