"""Windowed-sinc resampling at arbitrary ratio on the device: the polyphase tables (numpy), the 32.32 step
arithmetic, the host check of the kernel's tables, and `resample`, one launch of `mrmt3_resample_mix_fwd` over a 1-D
device tensor.  Pitch-shift rows (`mrmt3.batching.StemMixBatcher(pitch_shift=...)`), stems at their native rate and
`InferenceHandler.inference(sample_rate=...)` are built on it.  No CPU fallback: the kernel is the only implementation
(tests/_resample.py restates its contract in numpy for the tests).

A ratio is input samples per output sample (rate_in / rate_out; 2^(k/12) for a shift of k semitones) and travels as a
32.32 fixed-point `step`.  The step of 44100 / 16000 is rounded to 2^-32: a relative rate error of about 1e-10.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

PHASES = 512                    # ABI constant (include/mrmt3_hip.h): a table has PHASES + 1 rows
ONE = 1 << 32                   # step 1.0
MIN_RATIO, MAX_RATIO = Fraction(1, 4), Fraction(4)
MAX_TAPS = 160


def ratio_step(ratio) -> int:
    """round(ratio * 2^32) for a ratio in [1/4, 4] (a float, an int or a Fraction); anything else is a ValueError."""
    try:
        r = Fraction(ratio)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("resample ratio must be a finite number, got %r" % (ratio,)) from None
    if not MIN_RATIO <= r <= MAX_RATIO:
        raise ValueError("resample ratio must be in [1/4, 4], got %r" % (ratio,))
    return int(round(r * ONE))


def out_length(n_in: int, step: int) -> int:
    """Outputs whose position i * step lies on or before the last input sample."""
    return ((int(n_in) - 1) << 32) // int(step) + 1


def resample_filter(ratio, zeros: int = 16, beta: float = 8.6, rolloff: float = 0.94) -> np.ndarray:
    """float32 [513, T] polyphase table of a Kaiser-windowed sinc for `ratio` input samples per output sample:
    fc = rolloff * min(1, 1 / ratio), half = ceil(zeros / fc), T = 2 * half,
    h[p][t] = fc * sinc(fc * x) * kaiser_beta(x / half) for |x| < half else 0, x = (t - half + 1) - p / 512
    (row 512 is row 0 shifted by one sample).  Computed in float64, rounded to f32 once."""
    ratio = float(ratio)
    fc = rolloff * min(1.0, 1.0 / ratio)
    half = int(math.ceil(zeros / fc))
    T = 2 * half
    if T > MAX_TAPS:
        raise ValueError("resample filter for ratio %r needs %d taps, the kernel takes %d" % (ratio, T, MAX_TAPS))
    x = (np.arange(T, dtype=np.float64)[None, :] - half + 1) - np.arange(PHASES + 1, dtype=np.float64)[:, None] / PHASES
    inside = np.abs(x) < half
    u = np.where(inside, x / half, 0.0)
    h = fc * np.sinc(fc * x) * np.i0(beta * np.sqrt(1.0 - u * u)) / np.i0(beta)
    return np.where(inside, h, 0.0).astype(np.float32)


def stack_filters(tables) -> np.ndarray:
    """Tables of unequal T as one float32 [n, 513, Tmax]: each zero-padded symmetrically to the widest."""
    T = max(t.shape[1] for t in tables)
    out = np.zeros((len(tables), PHASES + 1, T), np.float32)
    for i, t in enumerate(tables):
        pad = (T - t.shape[1]) // 2
        out[i, :, pad:pad + t.shape[1]] = t
    return out


def check_resample_tables(src_pos, src_begin, src_end, src_step, src_gain, src_filt, pool_samples: int, n_filt: int):
    """Host check of the kernel's tables before they are uploaded (the companion of `check_mix_tables`): one
    [rows, sources] shape, 1 to 64 sources; every gain finite; for every source that sounds (gain != 0)
    0 <= begin <= end <= pool_samples, begin <= pos >> 32 <= end, the step in [2^30, 2^34], filt in [-1, n_filt), and
    filt = -1 only together with step 2^32 and a zero fraction.  A ValueError names the row.  (The kernel is safe without
    it; a table that needs the kernel's clamps is a planning bug.)"""
    pos, begin, end, step = (np.asarray(a, np.int64) for a in (src_pos, src_begin, src_end, src_step))
    gain, filt = np.asarray(src_gain, np.float32), np.asarray(src_filt, np.int64)
    shapes = [a.shape for a in (pos, begin, end, step, gain, filt)]
    if not (all(s == shapes[0] for s in shapes) and gain.ndim == 2):
        raise ValueError("resample tables: pos, begin, end, step, gain and filt must share one [rows, sources] shape, got %s"
                         % (shapes,))
    if not 1 <= gain.shape[1] <= 64:
        raise ValueError("resample tables: %d sources per row, the kernel takes 1 to 64" % gain.shape[1])
    for b in range(gain.shape[0]):
        if not np.isfinite(gain[b]).all():
            raise ValueError("resample tables: row %d has a gain that is not finite: %s" % (b, gain[b].tolist()))
        on = gain[b] != 0
        p, bg, en, st, fl = pos[b][on], begin[b][on], end[b][on], step[b][on], filt[b][on]
        if (bg < 0).any() or (bg > en).any() or (en > pool_samples).any():
            raise ValueError("resample tables: row %d points outside the pool of %d samples (begin %s, end %s)"
                             % (b, pool_samples, bg.tolist(), en.tolist()))
        if ((p >> 32) < bg).any() or ((p >> 32) > en).any():
            raise ValueError("resample tables: row %d starts outside its stem (position %s, begin %s, end %s)"
                             % (b, (p >> 32).tolist(), bg.tolist(), en.tolist()))
        if (st < ONE // 4).any() or (st > ONE * 4).any():
            raise ValueError("resample tables: row %d has a step outside [1/4, 4]: %s" % (b, (st / ONE).tolist()))
        if (fl < -1).any() or (fl >= n_filt).any():
            raise ValueError("resample tables: row %d names a filter outside [-1, %d): %s" % (b, n_filt, fl.tolist()))
        if ((fl == -1) & ((st != ONE) | ((p & (ONE - 1)) != 0))).any():
            raise ValueError("resample tables: row %d passes a source through (filter -1) at a step other than 1 or a "
                             "fractional position (step %s, position %s)" % (b, st.tolist(), p.tolist()))


_filters = {}                   # (step, device) -> [1, 513, T] f32 on the device


def device_filter(step: int, device):
    """The table of `resample_filter(step / 2^32)` on `device` as [1, 513, T], uploaded once per (step, device)."""
    import torch
    key = (int(step), str(torch.device(device)))
    if key not in _filters:
        if len(_filters) >= 64:
            _filters.pop(next(iter(_filters)))
        _filters[key] = torch.from_numpy(resample_filter(Fraction(int(step), ONE))[None]).to(device)
    return _filters[key]


def resample(x_dev, rate_in, rate_out=16000):
    """A 1-D f32 device tensor at `rate_in` -> the same signal at `rate_out`, `out_length(n, step)` samples, in one
    launch (batch 1, one source, gain 1).  `rate_in == rate_out` returns its input."""
    import torch
    from mrmt3 import lib
    if rate_in == rate_out:
        return x_dev
    if not x_dev.is_cuda:
        raise RuntimeError("resample needs a device tensor (no CPU fallback)")
    if x_dev.dim() != 1 or x_dev.numel() < 1:
        raise ValueError("resample takes a non-empty 1-D tensor, got shape %s" % (tuple(x_dev.shape),))
    step = ratio_step(Fraction(rate_in) / Fraction(rate_out))
    x = x_dev.contiguous().float()
    n = x.numel()
    dev = x.device
    i64 = lambda v: torch.tensor([[v]], dtype=torch.int64, device=dev)
    out = lib.resample_mix(x, i64(0), i64(0), i64(n), i64(step), torch.ones(1, 1, device=dev),
                           torch.zeros(1, 1, dtype=torch.int32, device=dev), out_length(n, step), device_filter(step, dev))
    return out[0]
