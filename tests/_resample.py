"""The resampler's contract of include/mrmt3_hip.h (mrmt3_resample_mix_fwd) restated in numpy, and the constructions the
resampler tests share (tests/test_resample_cpu.py, tests/test_resample_gpu.py).  numpy only at import; nothing here
touches the library.

`resample_rows` is the contract, not the kernel: numpy rounds every f32 operation (there is no fused multiply-add to be
had), the taps are added in tap order and the sources in source order, a tap outside its stem is not added at all.
"""
import numpy as np

F32 = np.float32
PHASES = 512
ONE = 1 << 32


def resample_rows(pool, src_pos, src_begin, src_end, src_step, src_gain, src_filt, n_samples, filt, valid_samples=None):
    """float32 [B, n_samples].  pool float32 [P]; src_pos / src_begin / src_end / src_step int64 [B, K]; src_gain float32
    [B, K]; src_filt int [B, K]; filt float32 [n_filt, 513, T]."""
    pool = np.asarray(pool, F32)
    pos0, begin, end, step = (np.asarray(a, np.int64) for a in (src_pos, src_begin, src_end, src_step))
    gain, fidx = np.asarray(src_gain, F32), np.asarray(src_filt, np.int64)
    filt = np.asarray(filt, F32)
    n_filt, rows_p, T = filt.shape
    assert rows_p == PHASES + 1 and T % 2 == 0
    B, K = gain.shape
    rows = np.zeros((B, n_samples), F32)
    for b in range(B):
        lim = n_samples if valid_samples is None else max(0, min(n_samples, int(valid_samples[b])))
        if lim == 0:
            continue
        i = np.arange(lim, dtype=np.int64)
        row = rows[b, :lim]
        for k in range(K):
            g = gain[b, k]
            if g == 0:
                continue                                     # not read at all
            f, st, bg, en = int(fidx[b, k]), int(step[b, k]), int(begin[b, k]), int(end[b, k])
            if f < -1 or f >= n_filt or st <= 0 or bg >= en:
                continue                                     # silent
            lo, hi = max(bg, 0), min(en, len(pool))
            if f == -1:
                idx = (int(pos0[b, k]) >> 32) + i
                ok = (idx >= lo) & (idx < hi)
                prod = (g * pool[idx[ok]]).astype(F32)
                row[ok] = (row[ok] + prod).astype(F32)
                continue
            with np.errstate(over="ignore"):
                pos = pos0[b, k] + i * np.int64(st)          # int64, wrapping
            n = pos >> 32
            fr = pos & np.int64(0xffffffff)
            j = fr >> 23
            w = (fr & np.int64(0x7fffff)).astype(F32) * F32(2.0 ** -23)      # 23 bits: exact
            acc = np.zeros(lim, F32)
            for t in range(T):
                h0, h1 = filt[f, j, t], filt[f, j + 1, t]
                d = (h1 - h0).astype(F32)
                m = (w * d).astype(F32)
                c = (h0 + m).astype(F32)
                idx = n + (t - T // 2 + 1)
                ok = (idx >= lo) & (idx < hi)
                prod = (c[ok] * pool[idx[ok]]).astype(F32)
                acc[ok] = (acc[ok] + prod).astype(F32)
            row[:] = (row + (g * acc).astype(F32)).astype(F32)
    return rows


def resample_1d(x, step, filt, n_out=None):
    """One signal through `resample_rows`: source 0 of row 0 at position 0, gain 1, the whole of `x` as its stem."""
    x = np.asarray(x, F32)
    if n_out is None:
        n_out = ((len(x) - 1) << 32) // int(step) + 1
    a = lambda v: np.array([[v]], np.int64)
    return resample_rows(x, a(0), a(0), a(len(x)), a(step), np.ones((1, 1), F32), a(0), n_out, np.asarray(filt, F32)[None])[0]


def resample_case(n_src, n_samples, steps, seed=0, passthrough=()):
    """Three rows of `n_src` sources over one pool whose stems lie end to end behind odd-sized NaN gaps (what no source
    may read is NaN), source k read at steps[k % len(steps)] from a start with a non-zero fraction (sources listed in
    `passthrough` at step 1, whole position, filter -1).  Row 0: source 0's stem ends INSIDE the row, and (with 5
    sources) source 3 has gain 0 and points into a gap.  Row 1: valid_samples is short.  Row 2: every source starts a few
    samples before its stem's end.  src_begin / src_end are the stems' own bounds, so the first and last taps of every
    stem fall outside and must be skipped.  Returns dict(pool, pos, begin, end, step, gain, filt_idx, valid_samples,
    n_samples); the filter index of a source is the index of its step in `steps`."""
    from _stem_mix import GAINS
    rs = np.random.RandomState(77 * n_src + n_samples % 991 + seed)
    B = 3
    shape = (B, n_src)
    pos, begin, end = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    step, fidx, gain = np.zeros(shape, np.int64), np.zeros(shape, np.int64), np.zeros(shape, F32)
    pieces, at = [], 0
    for b in range(B):
        for k in range(n_src):
            st = int(steps[k % len(steps)])
            thru = k in passthrough
            if thru:
                st = ONE
            need = ((n_samples * st) >> 32) + 2                      # input samples the row spans
            lead = int(rs.randint(0, 60))                            # samples of the stem before the row's start
            avail = need + int(rs.randint(1, 200))
            if b == 0 and k == 0:
                avail = need // 2 + 3
            if b == 2:
                avail = 5
            gap = 2 * int(rs.randint(3, 40)) + 1
            pieces.append(np.full(gap, np.nan, F32))
            at += gap
            pieces.append((rs.uniform(-1, 1, lead + avail) * 2.0 ** -(k % 3)).astype(F32))
            begin[b, k], end[b, k] = at, at + lead + avail
            frac = 0 if thru else int(rs.randint(1, 1 << 32))
            pos[b, k] = ((at + lead) << 32) + frac
            step[b, k] = st
            fidx[b, k] = -1 if thru else k % len(steps)
            gain[b, k] = F32(GAINS[(b + k) % len(GAINS)])
            at += lead + avail
    pieces.append(np.full(9, np.nan, F32))
    if n_src >= 5:
        gain[0, 3] = 0
        pos[0, 3], begin[0, 3], end[0, 3] = 2 << 32, 1, 8            # inside the first NaN gap: must not be read
    valid = np.array([n_samples, max(1, n_samples // 2 + 1), n_samples], np.int64)
    return dict(pool=np.concatenate(pieces), pos=pos, begin=begin, end=end, step=step, gain=gain, filt_idx=fidx,
                valid_samples=valid, n_samples=n_samples)


def tone_errors(resampler, freq, rate_in, rate_out, n_in, skip=400):
    """Max |resampler(unit sine at `freq`) - the analytic sine at the output times| with `skip` samples cut at each edge;
    a tone above rate_out / 2 compares to zero."""
    x = np.sin(2 * np.pi * freq * np.arange(n_in) / rate_in).astype(F32)
    y = np.asarray(resampler(x), np.float64)
    want = np.sin(2 * np.pi * freq * np.arange(len(y)) / rate_out) if freq < rate_out / 2 else np.zeros(len(y))
    return float(np.abs(y - want)[skip:len(y) - skip].max())
