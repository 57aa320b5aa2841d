"""Constructions, fp64 references and checkers of the per-element tests of the row-wise kernels of csrc/rowops.hip, embed.hip,
loss.hip, optim.hip and layout.hip (tests/test_exact_rows_gpu.py; proven on the CPU by tests/test_exact_rows_cpu.py).  Plain torch on whatever device the
tensors live on; nothing here touches the library.

A. Data movement: position-coded operands whose every value is exact in bf16, so a copy, a cast, a transpose or a gather
   must return them bit for bit; the awkward f32 -> bf16 conversions, each at each position of a quad.
B. Sums of small integers (embedding gradient, norm-weight gradient): every partial sum is exact in f32 whatever the
   order, so the result must equal the float64 sum.
C. RMSNorm, gated GELU, cross-entropy, token log-probability and AdamW against fp64 restatements of the documented formulas,
   EVERY element held to a bound derived from the kernel's operation chain.  All bounds are worst-case counts in units of
   u = 2^-24 (the unit roundoff of f32: one correctly rounded operation errs by at most u |result|; the hardware's exp, log
   and rsqrt are taken at one ulp = 2u) and of the project's own constants.  `TREE(n)` is the depth of a sum of n terms
   per lane followed by the 64-lane xor tree, the shape every row reduction of those sources has.
"""
import math

import torch

import _exact as ex

U = 2.0 ** -24                          # unit roundoff of f32
BF16_MIN_NORMAL_EXP = -126
F32_MIN_NORMAL = 2.0 ** -126            # results below it may be flushed or keep only a few bits
FAST_TANH_T = 2e-7                      # csrc/common.h: "fast_tanh ... absolute error <= 2e-7"
EW_GRID = 256 * 4096                    # common.h ew_blocks(): a launch has at most 4096 workgroups of 256 lanes
EW_SIZES = (4, 4 * (EW_GRID + 3))       # one quad; a grid-stride loop that wraps (with a ragged last pass)
EB_CHUNK = 32                           # embed.hip: sorted rows summed per workgroup of the embedding gradient


def TREE(n_per_lane):
    return n_per_lane + 6


# ---- checkers -----------------------------------------------------------------------------------------------------------------

def check_bound(name, got, ref, bound):
    """|got - ref| <= bound at EVERY element (fp64 comparison; a NaN or Inf in `got` where `ref` is finite is a failure).
    Returns the largest error / bound over the elements whose bound is positive (where it is zero the values must be
    equal).  The message names the worst element."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(bound.shape), (name, got.shape, ref.shape, bound.shape)
    g, r, b = got.double().reshape(-1), ref.double().to(got.device).reshape(-1), bound.double().to(got.device).reshape(-1)
    assert bool(torch.isfinite(r).all()) and bool((b >= 0).all()), name + ": the reference or its bound is not finite"
    err = (g - r).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)                 # x / 0 = inf for x > 0
    if ratio.numel() == 0:
        return 0.0
    i = int(ratio.argmax())
    worst = float(ratio[i])
    if not worst <= 1.0:
        cols = got.shape[-1] if got.dim() > 1 else 1
        raise AssertionError("%s: error %.4g > bound %.4g (ratio %.3g) at flat index %d (row %d, col %d): got %.9g, want %.9g; "
                             "%d of %d elements out" % (name, float(err[i]), float(b[i]), worst, i, i // cols, i % cols,
                                                        float(g[i]), float(r[i]), int((ratio > 1.0).sum()), ratio.numel()))
    return worst


def bits16(t):
    return t.contiguous().view(torch.int16)


def assert_same_bits(got, want, what):
    """Equality of the bit patterns (distinguishes -0 from +0; a NaN equals the same NaN)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    view = torch.int16 if got.element_size() == 2 else torch.int32
    ex.assert_equal_everywhere(got.contiguous().view(view), want.contiguous().view(view), what + " (bit patterns)")


# ---- A. position-coded operands -----------------------------------------------------------------------------------------------

CODE_MOD = 513                          # integers -256 .. 256


def position_coded(rows, cols, device="cpu", dtype=torch.float32):
    """value[r, c] = k * 2^e with k = ((7 c + 3 r) mod 513) - 256 and e = (r mod 8) - 3: an integer of at most 9 bits
    times a power of two, exact in bf16.  Inside a row 513 consecutive columns are all different; rows differ by their
    power of two and, at the same power (r + 8 j), by 24 j in k."""
    r = torch.arange(rows, device=device, dtype=torch.int64)[:, None]
    c = torch.arange(cols, device=device, dtype=torch.int64)[None, :]
    k = ((7 * c + 3 * r) % CODE_MOD) - 256
    return (k.double() * torch.pow(2.0, ((r % 8) - 3).double())).to(dtype)


def position_coded_flat(n, device="cpu", dtype=torch.float32):
    """The same code over a flat tensor read as rows of 64."""
    return position_coded((n + 63) // 64, 64, device, dtype).reshape(-1)[:n].contiguous()


# offsets by which a flat index is plausibly misrouted: a neighbour, a quad, a 16-byte group of bf16, a wave, a workgroup,
# one pass of the grid-stride loop
MISROUTES = (1, 2, 3, 4, 8, 64, 256, 1024, 4 * EW_GRID)

TRANSPOSE_SHAPES = [(1, 1), (33, 7), (31, 65), (384, 512)]
TRB_SHAPES = [(136, 72), (72, 200), (64, 64), (8, 8), (2048, 512)]        # transpose_batched, all dimensions multiples of 8
TRB_GAP = 64                                                             # sentinel elements between two destinations


def trb_table(shift):
    """Element offsets of the TRB_SHAPES matrices in one flat source and one flat destination buffer: every matrix starts at a
    multiple of 8 plus `shift` (0: the 16-byte path inside, the pair path on overhanging tiles; 2: the pair path;
    1: single elements), destinations TRB_GAP or more elements apart.  -> ([(src, dst, rows, cols)], total elements)"""
    recs, at = [], TRB_GAP
    for r, c in TRB_SHAPES:
        at = (at + 7) // 8 * 8 + shift
        recs.append((at, at, r, c))
        at += r * c + TRB_GAP
    return recs, at + TRB_GAP


def bf16_special_values():
    """f32 values whose conversion to bf16 is awkward; subnormals are apart (bf16_subnormal_values).  3.39e38 lies between
    the largest finite bf16 (3.3895e38) and the point half way to 2^128 (3.3961e38), so it rounds DOWN to the largest finite
    bf16; 3.4e38 lies above that point and becomes inf."""
    tie_down, tie_up = 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8                  # -> 1.0 and 1.015625: exact ties, to even
    f32_ulp = 2.0 ** -23
    bf16_max = float(torch.finfo(torch.bfloat16).max)
    vals = [tie_down, tie_up, -tie_down, -tie_up, tie_down + f32_ulp, tie_up - f32_ulp, tie_down - f32_ulp, bf16_max, -bf16_max,
            3.39e38, -3.39e38, float("inf"), float("-inf"), 0.0, -0.0, float("nan"), 3.4e38, -3.4e38]
    return torch.tensor(vals, dtype=torch.float32)


def bf16_subnormal_values():
    return torch.tensor([1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149), 1.1754942e-38, -1.1754942e-38, 2.0 ** -133 * 1.00390625],
                        dtype=torch.float32)


def quads_with_each_value_at_each_position(vals):
    """[4 * len(vals), 4] f32: row 4 i + q holds vals[i] at position q and 1.5, -2.5, 3.5 around it."""
    n = vals.numel()
    out = torch.tensor([1.5, -2.5, 3.5, 0.75], dtype=torch.float32).repeat(4 * n, 1)
    for i in range(n):
        for q in range(4):
            out[4 * i + q, q] = vals[i]
    return out


def check_bf16_conversion(got, src, what, subnormal=False):
    """`got` (bf16) against torch's CPU round-to-nearest-even of the f32 `src`: same bits, except that a NaN may be any NaN
    and, with `subnormal`, that a zero of the same sign is accepted too.  -> 'rne' / 'flushed' / 'mixed' for subnormals."""
    got, src = got.cpu().reshape(-1), src.cpu().reshape(-1)
    want = src.bfloat16()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what + ": NaN positions differ"
    g, w = bits16(got)[~nan], bits16(want)[~nan]
    if not subnormal:
        ex.assert_equal_everywhere(g, w, what)
        return "rne"
    tiny = (src[~nan].abs() < F32_MIN_NORMAL) & (src[~nan] != 0)
    zero = torch.where(src[~nan] < 0, torch.tensor(-32768, dtype=torch.int16), torch.tensor(0, dtype=torch.int16))
    rne, flushed = g == w, tiny & (g == zero)
    assert bool((rne | flushed).all()), (what, g[~(rne | flushed)].tolist(), w[~(rne | flushed)].tolist())
    if bool(rne[tiny].all()):
        return "rne"
    return "flushed" if bool((flushed & ~rne)[tiny & (w != zero)].all()) else "mixed"


def token_ids(labels, seq_len, shift, start_id, pad_id, vocab):
    """embed.hip token_at(): the id row r embeds (shifted right inside its sequence, -100 -> pad, clamped to the table)."""
    ids = labels.reshape(-1).clone()
    if shift:
        prev = torch.cat([ids[:1], ids[:-1]])
        t = torch.arange(ids.numel(), device=ids.device) % seq_len
        ids = torch.where(t == 0, torch.full_like(ids, start_id), prev)
        ids = torch.where(ids == -100, torch.full_like(ids, pad_id), ids)
    return ids.clamp(0, vocab - 1)


def labels_for(eff, shift, pad_id):
    """Labels of ONE sequence (seq_len = rows) that make row r embed eff[r]: -> (labels, start_id).  With `shift` the rows
    that embed `pad_id` get there through the -100 -> pad rule."""
    if not shift:
        return eff.clone(), 0
    lab = torch.cat([eff[1:], eff[:1]])
    return torch.where(lab == pad_id, torch.full_like(lab, -100), lab), int(eff[0])


def _mix(x):
    """oracle.dropout_ref.drop_mix on uint32 values held in int64 tensors (int64 products wrap; the low 32 bits are kept)."""
    m32, m24 = 0xFFFFFFFF, 0xFFFFFF
    x = x & m32
    x = x ^ (x >> 16)
    x = ((x & m24) * 0x7FEB35) & m32
    x = x ^ (x >> 15)
    x = ((x & m24) * 0x6CA68B) & m32
    return x ^ (x >> 16)


def keep_mask_torch(n, p, seed, stream, step=None, device="cpu"):
    """oracle.dropout_ref.keep_mask (the restatement of common.h drop_mask4) in torch, on `device`, for the large cases:
    -> (keep [n] bool, scale).  The key, the threshold and the scale are dropout_ref.make_drop's; the CPU tests prove the
    mask equal to dropout_ref.keep_mask's."""
    from oracle import dropout_ref as dr
    assert n % 4 == 0 and n < 2 ** 33
    key, thresh, scale = dr.make_drop(p, seed, stream, step)
    if thresh == 0:
        return torch.ones(n, dtype=torch.bool, device=device), 1.0
    m32 = 0xFFFFFFFF
    c = (torch.arange(n // 4, device=device, dtype=torch.int64) << 1) & m32          # (idx4 >> 31 is zero below 2^33 elements)
    h0 = _mix((key + ((c * 0x9E3779B1) & m32)) & m32)
    h1 = _mix((key + ((((c + 1) & m32) * 0x9E3779B1) & m32)) & m32)
    u = torch.stack([h0 & 0xFFFF, h0 >> 16, h1 & 0xFFFF, h1 >> 16], 1).reshape(-1)
    return u >= thresh, float(scale)


# ---- B. exact sums ------------------------------------------------------------------------------------------------------------

EB_ROWS_LIST = [1, 31, 33, 255, 257, 16384 + 17]
EB_VOCABS = [1536, 1391]
EB_DX, EB_START = 4, 100                # |dx| <= 4, |dtable start| <= 100
EB_RUNS = [32, 64, 31, 1, 33]           # per-id counts, in sorted order: runs that start and end on EB_CHUNK boundaries


def eb_widths(rows):
    return [4, 512, 1028] if rows <= 257 else [4, 512]


def eb_sum_bound(rows, scale=1.0):
    return rows * EB_DX * scale + EB_START


def eb_ids(layout, rows, vocab, seed):
    """Effective ids of `rows` rows (int64, CPU), shuffled so that the kernel's sort has work to do.
    'three': three ids (0, a middle one, vocab - 1) at random, every run crosses chunk boundaries once rows > 96;
    'runs': the first ids have EB_RUNS rows each (cut off at `rows`), the rest one id each per EB_CHUNK + 5 rows;
    'one': one id for all rows."""
    g = torch.Generator().manual_seed(seed)
    if layout == "three":
        ids = torch.tensor([0, vocab // 2 + 1, vocab - 1])[torch.randint(0, 3, (rows,), generator=g)]
    elif layout == "one":
        ids = torch.full((rows,), vocab - 7, dtype=torch.int64)
    else:
        counts = list(EB_RUNS)
        while sum(counts) < rows:
            counts.append(EB_CHUNK + 5)
        first = [3, 4, 17, 18, 40] + list(range(41, 41 + len(counts) - 5))           # ascending: the sorted order of the runs
        assert first[-1] < vocab
        ids = torch.cat([torch.full((n,), i, dtype=torch.int64) for n, i in zip(counts, first)])[:rows]
    return ids[torch.randperm(rows, generator=g)]


DW_ROWS = [1, 3, 5, 4097, 16383, 16384, 16385, 40001]
DW_COLS = [256, 512, 1024, 2048]
DW_X1, DW_G, DW_RSTD, DW_START = 8, 4, (0.5, 1.0, 2.0), 100
EXACT_HALVES = 2 ** 23                  # every multiple of 1/2 of magnitude <= 2^23 is an f32


def dw_cols_for(rows):
    return [512] if rows == 40001 else DW_COLS


def dw_sum_bound(rows, scale=1.0, passes=1):
    """Largest |partial sum| of dw[c] = sum_r dxn x1 rstd (multiples of 1/2) over `passes` accumulations onto the start."""
    return passes * rows * DW_G * DW_X1 * max(DW_RSTD) * scale + DW_START


def dw_case(rows, cols, device, seed, g_dtype=torch.float32):
    x1 = ex.rand_ints((rows, cols), -DW_X1, DW_X1, torch.float32, device, seed)
    dxn = ex.rand_ints((rows, cols), -DW_G, DW_G, g_dtype, device, seed + 1)
    pick = ex.rand_ints((rows,), 0, 2, torch.int64, device, seed + 2)
    rstd = torch.tensor(DW_RSTD, device=device, dtype=torch.float32)[pick]
    dw0 = ex.rand_ints((cols,), -DW_START, DW_START, torch.float32, device, seed + 3)
    return x1, rstd, dxn, dw0


def dw_reference(x1, rstd, dxn, dw0, keep=None, scale=1.0):
    g = dxn.double() if keep is None else dxn.double() * keep.double().reshape(dxn.shape) * scale
    return dw0.double() + (g * x1.double() * rstd.double()[:, None]).sum(0)


def dx1_integer_reference(x1, rstd, dxn, w):
    """fp64 dx1 of the integer case with a weight of ones: rstd (g - xh mean(g xh)); exact in f32 too (tests prove it)."""
    xh = x1.double() * rstd.double()[:, None]
    gw = dxn.double() * w.double()
    return rstd.double()[:, None] * (gw - xh * (gw * xh).mean(1, keepdim=True))


# ---- C. RMSNorm -----------------------------------------------------------------------------------------------------------------

NORM_EPS = 1e-6
NORM_ROWS = [1, 3, 5, 1000]
NORM_COLS = [256, 512, 1024, 2048]
NORM_KINDS = 5                          # zero, 1e-4, 1e6, spike, randn


def norm_case(rows, cols, first_kind=0, seed=0, device="cpu"):
    """x0, y (f32; every value of y is a bf16), w, dxn, dres (f32; dxn and dres hold bf16 values).  Row r is of kind
    (first_kind + r) mod 5 for r < 5 and Gaussian with a scale of its own after that:
      0  x0 + y is exactly zero everywhere (x0 = -y): rstd = eps^-1/2, xn = 0, dx1 = rstd w dxn + dres
      1  magnitude 1e-4: eps dominates the mean square
      2  magnitude 1e6
      3  one element of 1e4 among elements of 1e-3
      4  Gaussian"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * rows + cols + first_kind)
    row = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    scale = 2.0 ** (torch.arange(rows, dtype=torch.float64) % 11 - 5) * (1 + 0.01 * torch.arange(rows, dtype=torch.float64) / max(rows, 1))
    x1 = row * scale[:, None]
    zero_rows = []
    for r in range(min(rows, NORM_KINDS)):
        kind = (first_kind + r) % NORM_KINDS
        if kind == 0:
            zero_rows.append(r)
        elif kind == 1:
            x1[r] = row[r] * 1e-4
        elif kind == 2:
            x1[r] = row[r] * 1e6
        elif kind == 3:
            x1[r] = row[r] * 1e-3
            x1[r, (37 * (rows + cols)) % cols] = 1e4
    y = (0.25 * x1).float().bfloat16().float()
    x0 = (x1 - y.double()).float()
    for r in zero_rows:
        y[r] = torch.randn(cols, generator=g).bfloat16().float()
        x0[r] = -y[r]
    w = (1 + 0.1 * torch.randn(cols, generator=g)).float()
    w[1], w[cols // 2] = -0.75, 0.0
    dxn = torch.randn(rows, cols, generator=g).bfloat16().float()
    dres = torch.randn(rows, cols, generator=g).bfloat16().float()
    return tuple(t.to(device) for t in (x0, y, w, dxn, dres))


def rstd_rtol(cols):
    """Relative bound of rstd = rsqrt(ss / cols + eps), ss = sum of v^2 over the row, v = fl(x0 + y):
    v carries u, v^2 therefore 2u; the fma chain of cols/64 terms per lane and the wave tree add TREE(cols/64) u to the sum of
    positive terms; / cols is exact (a power of two); + eps: u.  Half of all that goes through the square root, and rsqrt
    itself is one ulp (2u)."""
    return (0.5 * (2 + TREE(cols // 64) + 1) + 2) * U


def norm_fwd_reference(x0, y, w, eps=NORM_EPS):
    """fp64 (x1, xn, rstd) of HF T5LayerNorm on x1 = x0 + y and the per-element bounds of the f32 kernel:
      x1   one addition: u |x1|
      rstd rstd_rtol(cols) |rstd|
      xn   = w (v rstd): v carries u, rstd its bound, two products 2u: (rstd_rtol + 3u) |xn|  (+ 2^-9 |xn| for a bf16 xn;
           the caller adds it)."""
    x1 = x0.double() if y is None else x0.double() + y.double()
    cols = x1.shape[1]
    rstd = torch.rsqrt((x1 * x1).mean(1) + eps)
    xn = w.double() * (x1 * rstd[:, None])
    return dict(x1=x1, rstd=rstd, xn=xn, x1_tol=U * x1.abs(), rstd_tol=rstd_rtol(cols) * rstd,
                xn_tol=(rstd_rtol(cols) + 3 * U) * xn.abs())


def norm_bwd_reference(dxn, dres, x1, rstd, w):
    """fp64 dx1 = rstd (gw - xh dot) + dres with gw = dxn w, xh = x1 rstd, dot = mean(gw xh) over the row, of the f32 INPUTS
    x1 and rstd the kernel is given, and the bound of the kernel's chain:
      gw, xh: one product each (u);  dot: products u, a sum of cols/64 fmas per lane and the wave tree, exact / cols:
      |d dot| <= (TREE(cols/64) + 2) u mean|gw xh| =: D;  the fma gw - xh dot rounds once; times rstd: u; plus dres: u.
      |d dx1| <= u [ rstd (3 |gw| + 4 |xh dot|) + |dx1| + |dres| ] + rstd |xh| D."""
    cols = x1.shape[1]
    xh = x1.double() * rstd.double()[:, None]
    gw = dxn.double() * w.double()
    prod = gw * xh
    dot = prod.mean(1, keepdim=True)
    r = rstd.double()[:, None]
    res = 0.0 if dres is None else dres.double()
    dx1 = r * (gw - xh * dot) + res
    D = (TREE(cols // 64) + 2) * U * prod.abs().mean(1, keepdim=True)
    tol = U * (r * (3 * gw.abs() + 4 * (xh * dot).abs()) + dx1.abs() + (0.0 if dres is None else res.abs())) + r * xh.abs() * D
    return dx1, tol


def bf16_half_ulp(x):
    """Half a bf16 ulp at |x|: 2^(floor(log2 |x|) - 8), bf16 keeping 8 significant bits (2^-134 below the normal range).
    It lies between 2^-9 |x| (just below a power of two) and 2^-8 |x| (at one): 2^-9 |x| alone is a bound that a correct
    rounding does not meet (1.0039 becomes 1.0, off by 2^-8.01 of itself)."""
    e = torch.frexp(x.double().abs())[1] - 1                          # |x| = m 2^(e + 1), 0.5 <= m < 1
    return torch.pow(2.0, (e.clamp(min=BF16_MIN_NORMAL_EXP) - 8).double())


def with_bf16(tol, ref):
    """Bound of a bf16 output: the f32 value y lies within `tol` of `ref` and is then rounded to nearest, which moves it by
    at most half a bf16 ulp of y, so of |ref| + tol."""
    return tol + bf16_half_ulp(ref.abs() + tol)


def norm_fwd_restated(x0, y, w, eps=NORM_EPS, fault=None):
    """The kernel's formula in torch f32, torch's own summation order.  Faults: 'eps_outside', 'mean_cols_minus_4'."""
    x1 = x0 if y is None else x0 + y
    cols = x1.shape[1]
    ss = (x1 * x1).sum(1)
    if fault == "eps_outside":
        rstd = 1.0 / (torch.sqrt(ss / cols) + eps)
    elif fault == "mean_cols_minus_4":
        rstd = torch.rsqrt(ss / (cols - 4) + eps)
    else:
        rstd = torch.rsqrt(ss / cols + eps)
    return x1, w * (x1 * rstd[:, None]), rstd


def norm_bwd_restated(dxn, dres, x1, rstd, w, drop_dot_row=None):
    xh = x1 * rstd[:, None]
    gw = dxn * w
    dot = (gw * xh).sum(1, keepdim=True) / x1.shape[1]
    if drop_dot_row is not None:
        dot[drop_dot_row] = 0.0
    return rstd[:, None] * (gw - xh * dot) + dres


# ---- C. gated GELU --------------------------------------------------------------------------------------------------------------

GELU_C, GELU_K = 0.7978845608028654, 0.044715
GEGLU_DFF = [8, 1024]
GEGLU_EXTRA = [0.0, 1e-30, -1e-30, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4]


def geglu_case(dff, dtype=torch.float32, device="cpu"):
    """h = [a | b] of [rows, 2 dff] and dg [rows, dff]: a walks 64 * 96 points over [-12, 12] and the GEGLU_EXTRA values
    (padded with 0.5 to whole rows), b and dg are +-2^x with x uniform in [-3, 3], different at every element."""
    a = torch.cat([torch.linspace(-12.0, 12.0, 64 * 96, dtype=torch.float64), torch.tensor(GEGLU_EXTRA, dtype=torch.float64)])
    rows = (a.numel() + dff - 1) // dff
    a = torch.cat([a, torch.full((rows * dff - a.numel(),), 0.5, dtype=torch.float64)]).reshape(rows, dff)
    g = torch.Generator().manual_seed(dff)
    def pm_pow2():
        x = torch.rand(rows, dff, generator=g, dtype=torch.float64) * 6 - 3
        return torch.pow(2.0, x) * (torch.randint(0, 2, (rows, dff), generator=g).double() * 2 - 1)
    h = torch.cat([a, pm_pow2()], 1).float().to(dtype)
    dg = pm_pow2().float().to(dtype)
    return h.to(device), dg.to(device)


def geglu_reference(h, dg=None):
    """fp64 g = gelu_new(a) b (HF NewGELUActivation, T5DenseGatedGeluDense) and, with dg, dh = [dg b gelu'(a) | dg gelu(a)],
    with the bounds that follow from common.h's statement that fast_tanh is within T = FAST_TANH_T absolute.
    The tanh t the kernel uses errs by dt <= 2T: T for fast_tanh itself, and T for its argument c (x + k x^3), which is
    rounded four times and uses f32 roundings of c and k (<= 6u relative; (1 - t^2) |arg| <= 0.45, so <= 2.7u < T).
      f  = 0.5 x (1 + t) (one fma), g = f b:     |dg| <= |b| (0.5 |x| 2T + 4u |f|)                       (the issue's bound)
      p  = 0.5 + 0.5 t:                          |dp| <= T + u
      q  = 1 - t^2 (one fma):                    |dq| <= 2 |t| 2T + (2T)^2 + u
      wq = 0.5 x c (1 + 3k x^2): three products and an fma, 3k rounded: 5u relative
      f' = p + wq q (one fma):                   |df'| <= |dp| + |wq| |dq| + 5u |wq q| + u |f'|
      da = (dg b) f': two products               |dda| <= |dg b| (|df'| + 2u |f'|)
      db = dg f:                                 |ddb| <= |dg| (0.5 |x| 2T + 4u |f|)"""
    dff = h.shape[1] // 2
    x, b = h[:, :dff].double(), h[:, dff:].double()
    T = FAST_TANH_T
    t = torch.tanh(GELU_C * (x + GELU_K * x ** 3))
    f = 0.5 * x * (1 + t)
    df_tol = 0.5 * x.abs() * 2 * T + 4 * U * f.abs()
    out = dict(g=f * b, g_tol=b.abs() * df_tol)
    if dg is not None:
        go = dg.double()
        q = 1 - t * t
        wq = 0.5 * x * GELU_C * (1 + 3 * GELU_K * x * x)
        fd = 0.5 * (1 + t) + wq * q
        dq = 2 * t.abs() * 2 * T + (2 * T) ** 2 + U
        dfd = (T + U) + wq.abs() * dq + 5 * U * (wq * q).abs() + U * fd.abs()
        out["dh"] = torch.cat([go * b * fd, go * f], 1)
        out["dh_tol"] = torch.cat([(go * b).abs() * (dfd + 2 * U * fd.abs()), go.abs() * df_tol], 1)
    return out


def geglu_restated(h, dg=None, fault=None):
    """common.h gelu_new_f / gelu_new_fd in torch f32 (fast_tanh = 1 - 2 / (exp2(2 log2(e) u) + 1)).
    Faults: 'k_0447' (0.044715 -> 0.0447), 'erf' (erf-GELU), 'no_q' (the derivative's q term dropped)."""
    dff = h.shape[1] // 2
    x, b = h[:, :dff].float(), h[:, dff:].float()
    k = 0.0447 if fault == "k_0447" else GELU_K
    arg = GELU_C * (k * (x * x * x) + x)
    t = 1.0 - 2.0 / (torch.exp2(arg * 2.885390081777927) + 1.0)
    f = 0.5 * x * t + 0.5 * x
    if fault == "erf":
        f = 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))
    if dg is None:
        return f * b
    q = 1.0 - t * t
    fd = (0.5 * x) * q * GELU_C * (3 * k * (x * x) + 1.0) * (0.0 if fault == "no_q" else 1.0) + (0.5 * t + 0.5)
    if fault == "erf":
        fd = 0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327
    go = dg.float()
    return f * b, torch.cat([go * b * fd, go * f], 1)


# ---- C. cross-entropy and token log-probability ------------------------------------------------------------------------------------

CE_VOCABS = [1536, 1100, 200]           # the wave kernel; the block kernel; the block kernel with three idle waves
CE_ROWS = [1, 37]
CE_BIG = (24577, 1536)                  # ce_rows_per_wave = 3, the last wave's walk is cut short
CE_KINDS = 8
CE_MARGIN = 60.0
CE_EPS, CE_Z, CE_GRAD_SCALE = 0.1, 1e-4, 0.5


def ce_wave_kernel_takes(V):
    return V in (512, 1024, 1536, 2048)


def ce_tie_columns(V):
    """Four columns of one row that sit in different lanes and, in the block kernel, different waves."""
    return sorted({(4 * 1 + 1) % V, (4 * 70 + 2) % V, (4 * 135 + 3) % V, V - 1 - 4 * 3}) if V > 16 else list(range(min(V, 4)))


def logits_case(rows, V, first_kind=0, seed=0, device="cpu", ignore_every=5, inst=(None, None)):
    """f32 logits [rows, V] and int64 targets.  Row r is of kind (first_kind + r) mod 8:
      0 offset +1e4   1 offset -1e4   2 one dominant logit (CE_MARGIN above the rest)   3 the maximum tied at four columns
      4 maximum at column 0   5 maximum at column V - 1   6, 7 Gaussian (scale 2)
    targets: random, 0 and V - 1 forced on rows 8 j + 6 and 8 j + 7 and (when given) a few inside inst = (lo, hi);
    every `ignore_every`-th row (r mod 5 == 4) is -100."""
    g = torch.Generator().manual_seed(7 * rows + V + 100 * first_kind + seed)
    l = torch.randn(rows, V, generator=g) * 2
    r = torch.arange(rows)
    kind = (first_kind + r) % CE_KINDS
    top = l.max(1).values
    l[kind == 0] += 1e4
    l[kind == 1] -= 1e4
    hot = torch.randint(0, V, (rows,), generator=g)
    sel = kind == 2
    l[sel, hot[sel]] = top[sel] + CE_MARGIN
    for c in ce_tie_columns(V):
        l[kind == 3, c] = top[kind == 3] + 1.0
    l[kind == 4, 0] = top[kind == 4] + 0.5
    l[kind == 5, V - 1] = top[kind == 5] + 0.5
    t = torch.randint(0, V, (rows,), generator=g)
    t[sel] = torch.where(torch.rand(int(sel.sum()), generator=g) < 0.5, hot[sel], t[sel])       # on and off the dominant logit
    t[kind == 6] = 0
    t[kind == 7] = V - 1
    if inst[0] is not None:
        t[r % 3 == 1] = inst[0] + (r[r % 3 == 1] % (inst[1] - inst[0] + 1))
    if ignore_every:
        t[r % ignore_every == ignore_every - 1] = -100
    return l.to(device), t.to(device)


def ce_reference(logits, targets, weighted, inst_lo, inst_hi, grad_scale=1.0, eps=0.0, z=0.0, grad_bf16=False):
    """fp64 loss, NLL and dlogits of tasks/mt3_net.py's (weighted) cross-entropy with label smoothing eps and z-loss z
    (loss.hip, REG): per scored row r = (1 - eps) nll + eps (lse - mean l) + z lse^2, loss = sum w r / denom,
    dlogits = g0 (p (1 + 2 z lse) - (1 - eps) [j = t] - eps / V), g0 = w grad_scale / denom; ignored rows: exactly zero.

    Bounds of the f32 kernels (mx = row maximum, se = sum exp(l - mx), p = exp(l - mx) / se, A = sum_j p_j |l_j - mx|):
      exp(l_j - mx): the subtraction rounds (u |l_j - mx| absolute in the exponent), exp is one ulp: (|l_j - mx| + 2) u
      se: those errors weighted by p (A + 2) u, and the sum of V positive terms in a tree of depth <= 4 ceil(V / 256) + 16
          (wave kernel: TREE(V / 64); block kernel: the running sums of a thread, the wave tree, four waves)
      the block kernel forms lse = mx + log(se) and p = exp(l - lse): lse rounds at u |lse| (an offset row pays for its
          offset here), log is one ulp (2u |log se|), l - lse rounds at u |l - lse|
      g0, (1 + 2 z lse), the products and the two subtractions: 10u on p and 4u on each subtracted term.
    So with C = 4 ceil(V / 256) + 32 and kappa = 1 for the block kernel, 0 for the wave kernel:
      |d dlogits_j| <= |g0| u [ p_j |pz| (C + |l_j - mx| + A + 2 |log se| + kappa (|lse| + |l_j - lse|)) + 4 (p_j |pz| + eps / V + (1 - eps) [j = t]) ]
    and per row |d nll| <= u (|lse| + 2 |log se| + A + C + |l_t| + 4 |nll|); the smoothing term adds
      eps u (TREE(V / 64) + 4) mean|l| (the f32 sum of the raw logits) and the z term z (4u lse^2 + 2 |lse| d lse).
    The loss sums w r / denom over the rows: the bounds add up, plus 8u |loss| for 1 / denom, the f32 running sum of a
    wave's rows and the final conversion to f32."""
    l = logits.double()
    rows, V = l.shape
    t = targets
    scored = t != -100
    tt = t.clamp(min=0)
    w = scored.double()
    n = scored.double()
    if weighted:
        inst = scored & (t >= inst_lo) & (t <= inst_hi)
        w = torch.where(inst, torch.full_like(w, 3.0), w)
        n = torch.where(inst, torch.full_like(n, 2.0), n)
    denom = n.sum()
    mx = l.max(1, keepdim=True).values
    ex_ = torch.exp(l - mx)
    se = ex_.sum(1, keepdim=True)
    p = ex_ / se
    lse = mx + torch.log(se)
    lt = l.gather(1, tt[:, None])
    nll = (lse - lt)
    smooth = lse - l.mean(1, keepdim=True)
    r = (1 - eps) * nll + eps * smooth + z * lse * lse
    wd = (w / denom)[:, None]
    loss = float((wd * r).sum())
    loss_nll = float((wd * nll).sum())
    g0 = wd * grad_scale
    pz = 1 + 2 * z * lse
    onehot = torch.zeros_like(l).scatter_(1, tt[:, None], 1.0)
    dl = g0 * (p * pz - (1 - eps) * onehot - eps / V)
    A = (p * (l - mx).abs()).sum(1, keepdim=True)
    C = 4 * math.ceil(V / 256) + 32
    kappa = 0.0 if ce_wave_kernel_takes(V) else 1.0
    logse = torch.log(se).abs()
    apz = pz.abs()                                            # (an offset of -1e4 makes 1 + 2 z lse negative)
    dl_tol = g0.abs() * U * (p * apz * (C + (l - mx).abs() + A + 2 * logse + kappa * (lse.abs() + (l - lse).abs()))
                             + 4 * (p * apz + eps / V + (1 - eps) * onehot))
    if grad_bf16:
        dl_tol = with_bf16(dl_tol, dl)
    d_lse = U * (lse.abs() + 2 * logse + A + C)
    d_nll = d_lse + U * (lt.abs() + 4 * nll.abs())
    d_r = (1 - eps) * d_nll + eps * (d_lse + U * (TREE(V // 64) + 4) * l.abs().mean(1, keepdim=True)) + \
        z * (4 * U * lse * lse + 2 * lse.abs() * d_lse) + 4 * U * r.abs()
    loss_tol = float((wd * d_r).sum()) + 8 * U * abs(loss)
    nll_tol = float((wd * d_nll).sum()) + 8 * U * abs(loss_nll)
    return dict(loss=loss, nll=loss_nll, dl=dl, dl_tol=dl_tol, loss_tol=loss_tol, nll_tol=nll_tol, scored=scored)


def ce_restated(logits, targets, weighted, inst_lo, inst_hi, grad_scale=1.0, eps=0.0, z=0.0, block=False):
    """The kernels' formulas in torch f32: p = exp(l - mx) / se (wave kernel) or exp(l - (mx + log se)) (block kernel)."""
    l = logits.float()
    rows, V = l.shape
    scored = targets != -100
    tt = targets.clamp(min=0)
    w = scored.float()
    n = scored.float()
    if weighted:
        inst = scored & (targets >= inst_lo) & (targets <= inst_hi)
        w, n = torch.where(inst, torch.full_like(w, 3.0), w), torch.where(inst, torch.full_like(n, 2.0), n)
    inv_den = 1.0 / n.sum()
    mx = l.max(1, keepdim=True).values
    e = torch.exp(l - mx)
    se = e.sum(1, keepdim=True)
    lse = mx + torch.log(se)
    p = torch.exp(l - lse) if block else e / se
    nll = lse - l.gather(1, tt[:, None])
    r = (1 - eps) * nll + eps * (lse - l.sum(1, keepdim=True) * (1.0 / V)) + z * lse * lse
    g0 = (w * inv_den * grad_scale)[:, None]
    onehot = torch.zeros_like(l).scatter_(1, tt[:, None], 1.0)
    dl = g0 * ((p * (1 + 2 * z * lse) - eps / V) - (1 - eps) * onehot)
    return float((w[:, None] * r * inv_den).double().sum()), float((w[:, None] * nll * inv_den).double().sum()), dl


TLP_VOCABS = [1, 5, 1391, 1536, 2048]
TLP_ROWS = [1, 6]


def logprob_reference(logits, targets, ignore_index=-100):
    """fp64 log_softmax(l)[t] (0 at an ignored row, NaN for a row that holds a NaN) and the bound of
    loss.hip token_logprob = (l_t - mx) - log(se): the subtraction u |l_t - mx|, se as in ce_reference with a chain of
    32 terms per lane and the wave tree, log one ulp, the last subtraction u |result|:
      |d| <= u (2 |l_t - mx| + A + TREE(32) + 4 + 2 |log se| + |result|)."""
    l = logits.double()
    scored = targets != ignore_index
    tt = targets.clamp(min=0)
    ref = torch.log_softmax(l, 1).gather(1, tt[:, None])[:, 0]
    mx = l.max(1, keepdim=True).values
    e = torch.exp(l - mx)
    se = e.sum(1, keepdim=True)
    A = (e / se * (l - mx).abs()).sum(1)
    lt = l.gather(1, tt[:, None])[:, 0]
    tol = U * (2 * (lt - mx[:, 0]).abs() + A + TREE(32) + 4 + 2 * torch.log(se[:, 0]).abs() + ref.abs())
    ref = torch.where(scored, ref, torch.zeros_like(ref))
    tol = torch.where(scored, tol, torch.zeros_like(tol))
    return ref, tol


# ---- C. AdamW -------------------------------------------------------------------------------------------------------------------

ADAM = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_WD = [0.0, 0.1]
ADAM_GSCALE = [1.0, 1.0 / 3.0]
ADAM_SCENARIOS = [(0, 3), (100000, 2)]  # (step counter at the start, steps)


def f32(x):
    """The f32 the C ABI receives for the Python float x, as a Python float."""
    return float(torch.tensor(x, dtype=torch.float32))


def adam_case(n, step0, n_steps, device="cpu", seed=0):
    """p0, m0, v0 [n] f32 and grads [n_steps, n] f32.  Element i has gradient kind i mod 4 on every step: Gaussian, exactly
    zero (m0 = v0 = 0 there: the update must be the decay alone), 1e-20 (v underflows, the denominator is eps), 1e15."""
    g = torch.Generator(device=device).manual_seed(seed + n % 1000 + step0)
    p0 = torch.randn(n, device=device, generator=g)
    grads = torch.randn(n_steps, n, device=device, generator=g)
    kind = torch.arange(n, device=device) % 4
    grads[:, kind == 1] = 0.0
    grads[:, kind == 2] = 1e-20
    grads[:, kind == 3] = 1e15
    grads[1:, kind == 3] *= -0.5
    if step0 == 0:
        m0, v0 = torch.zeros(n, device=device), torch.zeros(n, device=device)
    else:
        m0 = torch.randn(n, device=device, generator=g) * 0.01
        v0 = torch.rand(n, device=device, generator=g) * 1e-4 + 1e-8
        m0[kind == 1], v0[kind == 1] = 0.0, 0.0
    return p0, m0, v0, grads


def adam_reference(p0, m0, v0, grads, step0, wd, gscale):
    """torch.optim.AdamW on float64 copies, given the SAME numbers the kernel is given (the f32 values of lr, the betas,
    eps, the weight decay and grad_scale), and per-element bounds of optim.hip adamw_kernel carried along the steps:
      gr = g gscale                                   u |gr|
      m' = m + (gr - m) c1   (c1 = 1 - beta1, exact)  em' = beta1 em + u (c1 |gr| + 2 c1 |gr - m| + |m'|)
      v' = v beta2 + (c2 gr) gr                       relative: rv' = rv + 5u   (a sum of non-negative terms; below
                                                      2^-126 v' may be flushed: + 2^-126 absolute)
      den = sqrt(v') / sqrt(bc2) + eps                relative rd = rv' / 2 + 4u + 2^-126 / v' influence, which eps swamps
      upd = step_size (m' / den)                      |d upd| <= step_size (em' + |m'| (rd + 3u)) / den
      p' = p decay - upd                              ep' = ep + 3u |p| + |d upd| + u |p'|   (decay = 1 - lr wd: u)
    -> list per step of dict(p, m, v, p_tol, m_tol, v_tol) in fp64."""
    lr, b1, b2, eps, wdf, gs = f32(ADAM["lr"]), f32(ADAM["beta1"]), f32(ADAM["beta2"]), f32(ADAM["eps"]), f32(wd), f32(gscale)
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf, foreach=False)
    opt.state[p] = dict(step=torch.tensor(float(step0)), exp_avg=m0.double().clone(), exp_avg_sq=v0.double().clone())
    em, rv, ep = torch.zeros_like(p.data), torch.zeros_like(p.data), torch.zeros_like(p.data)
    c1 = 1.0 - b1
    out = []
    for k in range(grads.shape[0]):
        step = step0 + k + 1
        gr = grads[k].double() * gs
        m_old, p_old = opt.state[p]["exp_avg"].clone(), p.data.clone()
        p.grad = gr.clone()
        opt.step()
        m, v = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
        em = b1 * em + U * (c1 * gr.abs() + 2 * c1 * (gr - m_old).abs() + m.abs())
        rv = rv + 5 * U
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        den = v.sqrt() / math.sqrt(bc2) + eps
        rd = rv / 2 + 4 * U
        d_upd = (lr / bc1) * (em + m.abs() * (rd + 3 * U)) / den
        ep = ep + 3 * U * p_old.abs() + d_upd + U * p.data.abs()
        out.append(dict(p=p.data.clone(), m=m.clone(), v=v.clone(), p_tol=ep.clone(), m_tol=em.clone(),
                        v_tol=rv * v + F32_MIN_NORMAL))
    return out


def adam_restated(p0, m0, v0, grads, step0, wd, gscale, fault=None):
    """optim.hip adamw_kernel in torch f32.  Faults: 'no_bias2' (the second-moment bias correction left out; it matters in the
    first steps only), 'eps_inside' (eps added under the square root)."""
    lr, b1, b2 = torch.tensor(ADAM["lr"], dtype=torch.float32), torch.tensor(ADAM["beta1"], dtype=torch.float32), \
        torch.tensor(ADAM["beta2"], dtype=torch.float32)
    eps, wdt, gs = torch.tensor(ADAM["eps"], dtype=torch.float32), torch.tensor(wd, dtype=torch.float32), \
        torch.tensor(gscale, dtype=torch.float32)
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    out = []
    for k in range(grads.shape[0]):
        step = step0 + k + 1
        bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
        step_size = torch.tensor(float(lr) / bc1, dtype=torch.float32)
        bc2_sqrt = torch.tensor(1.0 if fault == "no_bias2" else math.sqrt(bc2), dtype=torch.float32)
        decay = 1.0 - lr * wdt
        gr = grads[k] * gs
        p = p * decay
        m = m + (gr - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * gr * gr
        den = torch.sqrt(v / (bc2_sqrt * bc2_sqrt) + eps) if fault == "eps_inside" else torch.sqrt(v) / bc2_sqrt + eps
        p = p - step_size * (m / den)
        out.append((p.clone(), m.clone(), v.clone()))
    return out


def adam_decay_f32(wd):
    """decay = 1 - lr * wd as the kernel forms it in f32 (a product and a subtraction; contraction is off in optim.hip)."""
    return 1.0 - torch.tensor(ADAM["lr"], dtype=torch.float32) * torch.tensor(wd, dtype=torch.float32)
