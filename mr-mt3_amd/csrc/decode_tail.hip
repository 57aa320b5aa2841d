// The last kernel(s) of a decode step (decode.hip), which turn the step's logits into the next input: the greedy argmax
// (banned or not, with or without log-probabilities), the sampled tail, beam search (select + KV-cache
// reorder); their entry points and mrmt3_dec_launch_tail.
#include "decode.h"

// argmax + EOS bookkeeping (models/t5.py:286-295) + embedding of the next token.  One wave per sequence,
// 8 sequences per workgroup; the workgroup that finishes last (agent-scope counter) folds the finished
// flags into the "all done" state and advances the step counter — every other workgroup has read it by then.
__device__ __forceinline__ void dec_step_close(int* state, int B, int p, int t, bool token_step) {
  // no __threadfence() (on gfx950: write-back + invalidate of the XCD's L2, which would drop the weights the next
  // step is about to reread): the finished flags are agent-scope atomic stores, complete before the counter is bumped
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int old = __hip_atomic_fetch_add(&state[ST_CNT], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (old != (int)gridDim.x - 1) return;
  __hip_atomic_store(&state[ST_CNT], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (token_step) {
    int all_done = 1;
    for (int b = 0; b < B; ++b) all_done &= __hip_atomic_load(&state[ST_FLAGS + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (all_done && !state[ST_ALL]) { state[ST_ALL] = 1; state[ST_FIN] = t; }
  }
  state[ST_T] = p + 1;
}

// torch.argmax order: NaN above every number (the first NaN wins), then the larger value, then the lower index;
// index -1 = no candidate.  For finite logits this is the first maximum.
__device__ __forceinline__ bool argmax_beats(float v, int i, float bv, int bi) {
  if (i < 0) return false;
  if (bi < 0) return true;
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (!vn && v != bv) return v > bv;
  return i < bi;
}

// the row after the ban: banned columns and columns past V hold -inf
template <bool BAN>
__device__ __forceinline__ void load_row(float (&rl)[LOGP_REGS], const float* __restrict__ lrow, int V, int lane,
                                         const uint8_t* __restrict__ ban) {
#pragma unroll
  for (int i = 0; i < LOGP_REGS; ++i) {
    const int col = lane + 64 * i;
    rl[i] = (col < V) ? lrow[col] : -INFINITY;
  }
  if (BAN) {
#pragma unroll
    for (int i = 0; i < LOGP_REGS; ++i)
      if (lane + 64 * i < V && ban[lane + 64 * i]) rl[i] = -INFINITY;
  }
}
// its argmax (ascending column per lane, then the xor tree): best = l[idx] in every lane
__device__ __forceinline__ void argmax_row(const float (&rl)[LOGP_REGS], int V, int lane, float& best, int& idx) {
  float bv = -INFINITY;                  // accumulated in locals, not through the references: one chain of selects
  int bi = -1;                           // -1: this lane has seen no logit yet (lanes >= V when V < 64)
#pragma unroll
  for (int i = 0; i < LOGP_REGS; ++i) {
    const int col = lane + 64 * i;
    if (argmax_beats(rl[i], col < V ? col : -1, bv, bi)) { bv = rl[i]; bi = col; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (argmax_beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  best = bv;
  idx = bi;
}
// its log-softmax sums: mx the NaN-propagating maximum, se (SUM) the sum of exp(l - mx), per lane in ascending
// index then the xor tree; log p(c) = (l[c] - mx) - log(se).  -inf columns add exp(-inf) = 0.
template <bool SUM>
__device__ __forceinline__ void row_logsumexp(const float (&rl)[LOGP_REGS], float& mx, float& se) {
  mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < LOGP_REGS; ++i) mx = nanmax(mx, rl[i]);
  mx = wave_nanmax(mx);
  se = 0.f;
  if (SUM) {
#pragma unroll
    for (int i = 0; i < LOGP_REGS; ++i) se += expf(rl[i] - mx);
    se = wave_sum(se);
  }
}

// ---- what the greedy and the sampled tail share -------------------------------------------------------------------
// A step inside the prefix (p + 1 <= npre): the next input is the next memory row, or the start token right after the last
// one (models/t5_segmem.py:203-213); this step's logits are discarded and nothing is drawn.  512 threads = DMODEL.
__device__ __forceinline__ void dec_prefix_step(int B, const int64_t* __restrict__ tokens, int tok_ld,
                                                const float* __restrict__ embed, const float* __restrict__ pos,
                                                float* __restrict__ x, int* __restrict__ state,
                                                const float* __restrict__ prefix, int p, int npre) {
  const int tid = threadIdx.x;
  for (int b = blockIdx.x * 8; b < min(B, (int)blockIdx.x * 8 + 8); ++b) {
    const float* er = (p + 1 < npre) ? prefix + ((size_t)b * npre + p + 1) * DMODEL
                                     : embed + (size_t)tokens[(size_t)b * tok_ld] * DMODEL;
    const float* pr = pos + (size_t)(p + 1) * DMODEL;
    x[b * DMODEL + tid] = er[tid] + pr[tid];
  }
  __syncthreads();
  if (tid == 0) dec_step_close(state, B, p, 0, false);
}
// The lane's share of the next position's positional row: it does not depend on the token, so a token step requests it
// (and the finished flag) before its argmax or draw.
__device__ __forceinline__ void dec_load_pos(float (&pv)[DMODEL / 64], const float* __restrict__ pos, int p, int lane) {
  const float* pr = pos + (size_t)(p + 1) * DMODEL;
#pragma unroll
  for (int c = 0; c < DMODEL / 64; ++c) pv[c] = pr[c * 64 + lane];
}
// Row b's epilogue of token step t, by its wave: the chosen `idx` (in [0, V): lane 0 always holds index 0) or pad for a
// row that had finished, the next input x = embedding + positional row, the EOS flag, the token and (LOGP) its
// log-probability, 0.0 for a pad.
template <bool LOGP>
__device__ __forceinline__ void dec_emit_row(int b, int t, int lane, int idx, float lp_tok, int was_done, int eos, int pad,
                                             const float (&pv)[DMODEL / 64], const float* __restrict__ embed,
                                             float* __restrict__ x, int* __restrict__ state, int64_t* __restrict__ tokens,
                                             int tok_ld, float* __restrict__ logp, int logp_ld) {
  const int nxt = was_done ? pad : idx;
  const float* er = embed + (size_t)nxt * DMODEL;
#pragma unroll
  for (int c = 0; c < DMODEL / 64; ++c) x[b * DMODEL + c * 64 + lane] = er[c * 64 + lane] + pv[c];
  if (lane == 0) {
    if (!was_done && nxt == eos) __hip_atomic_store(&state[ST_FLAGS + b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tokens[(size_t)b * tok_ld + t + 1] = nxt;
    if (LOGP) logp[(size_t)b * logp_ld + t + 1] = was_done ? 0.f : lp_tok;
  }
}

// The greedy tail.  BAN: banned tokens (ban[c] != 0, a device [V] uint8 mask) score -inf before the argmax, NaN included, as
// HF's NoBadWordsLogitsProcessor does ahead of the greedy argmax.  The unbanned kernel is this body with BAN = false.
// (`ban` is the last argument, so the unbanned instantiation keeps every other argument's offset and its code.)
// LOGP: the wave also writes the log-probability of the token it emits, logp[b * logp_ld + t + 1], and keeps
// its row in registers, so the row is still read once; without LOGP it streams the row eight values at a time.
// Prefix steps write nothing.  (`logp`, `logp_ld` come after `ban`.)
template <bool BAN, bool LOGP>
__global__ __launch_bounds__(512) void dec_argmax(const float* __restrict__ logits, int V, int B, int64_t* __restrict__ tokens,
                                                  int tok_ld, const float* __restrict__ embed, const float* __restrict__ pos,
                                                  float* __restrict__ x, int* __restrict__ state, int eos, int pad,
                                                  const float* __restrict__ prefix, const uint8_t* __restrict__ ban,
                                                  float* __restrict__ logp, int logp_ld, int ban_stride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = state[ST_T];            // position just processed
  const int npre = state[ST_NPRE];
  if (p + 1 <= npre) {
    dec_prefix_step(B, tokens, tok_ld, embed, pos, x, state, prefix, p, npre);
    return;
  }
  const int t = p - npre;               // token step
  const int b = blockIdx.x * 8 + wave;
  if (b < B) {
    const int was_done = state[ST_FLAGS + b];
    float pv[DMODEL / 64];
    dec_load_pos(pv, pos, p, lane);
    float best = -INFINITY, lp_tok = 0.f;
    int idx = -1;
    if (BAN) ban += (size_t)b * ban_stride;     // 0: one static mask; V: a mask per row (the event grammar's)
    if (LOGP) {
      float rl[LOGP_REGS], mx, se;
      load_row<BAN>(rl, logits + (size_t)b * V, V, lane, ban);
      argmax_row(rl, V, lane, best, idx);
      row_logsumexp<true>(rl, mx, se);
      lp_tok = (best - mx) - logf(se);
    } else {
      for (int c0 = lane; c0 < V; c0 += 512) {
        float lv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) lv[u] = (c0 + 64 * u < V) ? logits[(size_t)b * V + c0 + 64 * u] : -INFINITY;
        if (BAN) {
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (c0 + 64 * u < V && ban[c0 + 64 * u]) lv[u] = -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int c = c0 + 64 * u;
          if (argmax_beats(lv[u], c < V ? c : -1, best, idx)) { best = lv[u]; idx = c; }   // ascending c per lane
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (argmax_beats(ov, oi, best, idx)) { best = ov; idx = oi; }
      }
    }
    dec_emit_row<LOGP>(b, t, lane, idx, lp_tok, was_done, eos, pad, pv, embed, x, state, tokens, tok_ld, logp, logp_ld);
  }
  __syncthreads();
  if (tid == 0) dec_step_close(state, B, p, t, true);
}

// ---- sampled tail (HF 4.18 sample(): ban -> temperature -> top-k -> top-p -> multinomial) -------------
// One wave owns a row and keeps it in registers, as dec_argmax<., true> does.  Nothing is sorted: a float's bit pattern,
// sign-folded, orders as the float does, so the k-th largest value and the top-p cut value are each found by building
// that 32-bit key from its top bit down (32 rounds of compare + accumulate + one wave reduction), and the drawn column
// by building its index the same way.  Every decision is taken on wave-reduced values: no lane diverges, and the kept
// set does not depend on timing.  Probabilities are f64 (exp and sums): a cut that sits within f32 rounding of top_p
// would otherwise move a token in or out of the kept set.
static inline unsigned sample_seed_key(unsigned long long seed) {
  return (unsigned)seed ^ ((unsigned)(seed >> 32) * 0x9E3779B1u);
}
// 24 random bits, a pure function of (seed key, row of the launch, token step).  The pair (row, step) is the counter:
// both enter both mixes, so two rows whose first mix collides (drop_mix keeps 24 bits) still draw different streams.
__device__ __forceinline__ unsigned sample_u24(unsigned key, unsigned row, unsigned step) {
  const unsigned a = drop_mix(key + row * 0x9E3779B1u + step * 0xC2B2AE35u);
  return drop_mix(a + step * 0x85EBCA6Bu + row * 0x27D4EB2Fu + 0x7F4A7C15u) >> 8;
}
// unsigned key that orders as the float does (-0 = +0); no NaN reaches it
__device__ __forceinline__ unsigned sample_order_key(float v) {
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The draw.  rl: the lane's logits after the ban (column lane + 64 i, -inf past V; consumed), mx their maximum (finite).
// Returns the drawn column, the same in every lane, always one with a non-zero kept probability.
__device__ __forceinline__ int sample_draw(float (&rl)[LOGP_REGS], float mx, int V, int lane, const SampleCfg& c,
                                           unsigned row, unsigned step) {
  float smx = mx;
  if (c.temperature != 1.0f) {
#pragma unroll
    for (int i = 0; i < LOGP_REGS; ++i) rl[i] = rl[i] / c.temperature;      // correctly rounded: monotone, max -> max
    smx = mx / c.temperature;
  }
  unsigned key[LOGP_REGS];
#pragma unroll
  for (int i = 0; i < LOGP_REGS; ++i) key[i] = sample_order_key(rl[i]);
  // top-k: thr = the k-th largest key = the largest x with |{key >= x}| >= k.  Columns past V hold -inf: they count only
  // for x <= key(-inf), where nothing is removed anyway.  Ties with the k-th value stay.
  unsigned thr = 0u;
  if (c.top_k > 0 && c.top_k < V) {
    for (unsigned bit = 0x80000000u; bit; bit >>= 1) {
      const unsigned cand = thr | bit;
      int n = 0;
#pragma unroll
      for (int i = 0; i < LOGP_REGS; ++i) n += key[i] >= cand ? 1 : 0;
      if (wave_sum_i(n) >= c.top_k) thr = cand;
    }
  }
  double e[LOGP_REGS];                    // unnormalised kept probability, exp(l - max); the maximum's is 1
#pragma unroll
  for (int i = 0; i < LOGP_REGS; ++i) e[i] = key[i] >= thr ? exp((double)rl[i] - (double)smx) : 0.0;
  // top-p: column c stays iff G(key_c) <= top_p * Z1, G(x) = mass of the keys above x (non-increasing in x).  The cut
  // is the least x with G(x) <= P: one more than the largest x with G(x) > P.  A group of equal logits shares its key,
  // so it stays or goes whole; G(largest key) = 0, so the most likely token always stays.
  if (c.top_p < 1.0f) {
    double z1 = 0.0;
#pragma unroll
    for (int i = 0; i < LOGP_REGS; ++i) z1 += e[i];
    const double P = (double)c.top_p * wave_sum_d(z1);
    auto above = [&](unsigned x) {
      double g = 0.0;
#pragma unroll
      for (int i = 0; i < LOGP_REGS; ++i) g += key[i] > x ? e[i] : 0.0;
      return wave_sum_d(g);
    };
    unsigned cut = 0u;
    if (above(0u) > P) {
      unsigned y = 0u;
      for (unsigned bit = 0x80000000u; bit; bit >>= 1)
        if (above(y | bit) > P) y |= bit;
      cut = y + 1u;                       // above(0xFFFFFFFF) = 0 <= P: y never reaches the top
    }
#pragma unroll
    for (int i = 0; i < LOGP_REGS; ++i) e[i] = key[i] >= cut ? e[i] : 0.0;
  }
  // draw: the lowest column whose cumulative kept mass (ascending column) exceeds u * Z.  z = the number of leading
  // columns whose mass is still <= the target; a target that rounding puts past every column takes the last kept one.
  double zs = 0.0;
  int last = -1;
#pragma unroll
  for (int i = 0; i < LOGP_REGS; ++i) {
    zs += e[i];
    if (e[i] > 0.0) last = lane + 64 * i;
  }
  const double target = (double)sample_u24(c.key, row, step) * 0x1p-24 * wave_sum_d(zs);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  int z = 0;
  for (int bit = 64 * LOGP_REGS; bit; bit >>= 1) {
    const int cand = z | bit;
    double f = 0.0;
#pragma unroll
    for (int i = 0; i < LOGP_REGS; ++i) f += lane + 64 * i < cand ? e[i] : 0.0;
    if (wave_sum_d(f) <= target) z = cand;
  }
  return max(min(z, last), 0);         // last >= 0: the maximum's column always has mass
}

// A row's token and (LOGP) its log-probability: what dec_argmax<., LOGP> computes, the greedy winner replaced by the
// draw when `draw` and the row's maximum is finite.  A row that holds an unbanned NaN, or no finite maximum (every
// logit banned or -inf, or a +inf), keeps the greedy winner.  The log-probability is the greedy tail's: log_softmax of
// the logits after the ban, before temperature and filters, same sums in the same order.  lrow: the row in memory.
template <bool LOGP>
__device__ __forceinline__ void sample_token(float (&rl)[LOGP_REGS], const float* __restrict__ lrow, int V, int lane,
                                             bool draw, const SampleCfg& c, unsigned row, unsigned step, int& tok,
                                             float& lp) {
  float best, mx, se;
  argmax_row(rl, V, lane, best, tok);
  row_logsumexp<LOGP>(rl, mx, se);
  if (draw && mx == mx && fabsf(mx) != INFINITY) {
    tok = sample_draw(rl, mx, V, lane, c, row, step);
    best = lrow[tok];                     // a drawn column is never a banned one
  }
  lp = LOGP ? (best - mx) - logf(se) : 0.f;
}

// dec_argmax with the draw in place of the winner.  `samp` is a device record (mrmt3_decoder_set_sampling writes it on the
// stream): a replayed graph freezes its by-value arguments, the record's contents are read at every step.  Row b draws
// with counter (b, t).
template <bool BAN, bool LOGP>
__global__ __launch_bounds__(512) void dec_sample(const float* __restrict__ logits, int V, int B, int64_t* __restrict__ tokens,
                                                  int tok_ld, const float* __restrict__ embed, const float* __restrict__ pos,
                                                  float* __restrict__ x, int* __restrict__ state, int eos, int pad,
                                                  const float* __restrict__ prefix, const uint8_t* __restrict__ ban,
                                                  float* __restrict__ logp, int logp_ld, const SampleCfg* __restrict__ samp,
                                                  int ban_stride) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = state[ST_T];
  const int npre = state[ST_NPRE];
  if (p + 1 <= npre) {
    dec_prefix_step(B, tokens, tok_ld, embed, pos, x, state, prefix, p, npre);
    return;
  }
  const int t = p - npre;
  const int b = blockIdx.x * 8 + wave;
  if (b < B) {
    const int was_done = state[ST_FLAGS + b];
    const SampleCfg cfg = *samp;
    float pv[DMODEL / 64];
    dec_load_pos(pv, pos, p, lane);
    const float* lrow = logits + (size_t)b * V;
    float rl[LOGP_REGS];
    load_row<BAN>(rl, lrow, V, lane, BAN ? ban + (size_t)b * ban_stride : ban);
    int idx;
    float lp_tok;
    sample_token<LOGP>(rl, lrow, V, lane, !was_done, cfg, (unsigned)b, (unsigned)t, idx, lp_tok);
    dec_emit_row<LOGP>(b, t, lane, idx, lp_tok, was_done, eos, pad, pv, embed, x, state, tokens, tok_ld, logp, logp_ld);
  }
  __syncthreads();
  if (tid == 0) dec_step_close(state, B, p, t, true);
}

// The rule alone on a caller's [rows][V] logits (mrmt3_sample_logits): row r draws with counter (row0 + r, step).
template <bool BAN, bool LOGP>
__global__ __launch_bounds__(512) void sample_logits_kernel(const float* __restrict__ logits, int rows, int V,
                                                            const uint8_t* __restrict__ ban, SampleCfg cfg, unsigned step,
                                                            unsigned row0, int64_t* __restrict__ tokens_out,
                                                            float* __restrict__ logp_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 8 + wave;
  if (r >= rows) return;
  const float* lrow = logits + (size_t)r * V;
  float rl[LOGP_REGS];
  load_row<BAN>(rl, lrow, V, lane, ban);
  int idx;
  float lp_tok;
  sample_token<LOGP>(rl, lrow, V, lane, true, cfg, row0 + (unsigned)r, step, idx, lp_tok);
  if (lane == 0) {
    tokens_out[r] = idx;
    if (LOGP) logp_out[r] = lp_tok;
  }
}

__global__ void dec_sampling_set_kernel(SampleCfg* rec, SampleCfg v) { *rec = v; }

// ---- beam search tail (HF 4.18 beam_search + BeamSearchScorer, early_stopping=False, one hypothesis kept) --------
// Row r = g * k + j is beam j of group (input segment) g.  Per group the caller owns a record of BEAM_HREC int32:
//   [0] hypotheses held   [1] worst kept score (f32 bits; 1e9 while fewer than k)   [2] done   [3] length of the
//   chosen hypothesis (written by the finalize kernel)   then up to k + 1 entries {score (f32 bits), end step, row}.
// A hypothesis {score, end step e, row r} is the start token plus row r's tokens of steps 0..e-1, read back through
// the backpointers bp[s][r] = {parent row, token} (int32 [max_len][rows][2]).
#define BEAM_MAXK 8
#define BEAM_HREC 32
#define BEAM_HYP0 4

// BeamHypotheses.add: the list keeps insertion order; past k entries the lowest score leaves (the earliest of equal
// lowest scores, as sorted((score, index))[0] picks), and the worst score becomes the lowest of the rest.
__device__ void beam_hyp_add(int* rec, int k, float score, int end_step, int row) {
  int n = rec[0];
  float worst = __int_as_float(rec[1]);
  if (!(n < k || score > worst)) return;
  int* e = rec + BEAM_HYP0 + 3 * n;
  e[0] = __float_as_int(score); e[1] = end_step; e[2] = row;
  ++n;
  if (n > k) {
    int lo = 0;
    for (int i = 1; i < n; ++i)
      if (__int_as_float(rec[BEAM_HYP0 + 3 * i]) < __int_as_float(rec[BEAM_HYP0 + 3 * lo])) lo = i;
    for (int i = lo; i + 1 < n; ++i)
      for (int f = 0; f < 3; ++f) rec[BEAM_HYP0 + 3 * i + f] = rec[BEAM_HYP0 + 3 * (i + 1) + f];
    --n;
    worst = __int_as_float(rec[BEAM_HYP0]);
    for (int i = 1; i < n; ++i) worst = fminf(worst, __int_as_float(rec[BEAM_HYP0 + 3 * i]));
  } else {
    worst = (worst < score) ? worst : score;
  }
  rec[0] = n;
  rec[1] = __float_as_int(worst);
}

// (value, index) pair that ranks first in argmax_beats order; index -1 = none.
__device__ __forceinline__ void rank_reduce_wave(float& v, int& i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    if (argmax_beats(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// One workgroup (8 waves) per group.  The k rows' log-softmax (+ ban, + beam score) fill LDS ([k][V] f32), the top 2k
// of those k*V candidates come out one per round (round r takes the best candidate ranked below round r-1's winner, so
// nothing is marked; order: score descending, NaN first, then flat index beam * V + token ascending), then lane 0
// walks them as BeamSearchScorer.process does.  The workgroup writes every row's next token, parent and score, the
// backpointers of step t, the next input x[row] = embed[token] + pos[t + 1] and, for a group that is done, the
// finished flags of its rows; the last workgroup folds them into ST_ALL / ST_FIN and advances the step.
__global__ __launch_bounds__(512) void dec_beam_select(const float* __restrict__ logits, int V, int k, int rows,
                                                       int64_t* __restrict__ tokens, int tok_ld,
                                                       const float* __restrict__ embed, const float* __restrict__ pos,
                                                       float* __restrict__ x, int* __restrict__ state, int eos, int pad,
                                                       float length_penalty, const uint8_t* __restrict__ ban,
                                                       float* __restrict__ bscore, int* __restrict__ bp,
                                                       int* __restrict__ hyp, float* __restrict__ blp,
                                                       size_t blp_plane, int ban_stride) {
  extern __shared__ float sc[];                 // [k][V] candidate scores
  __shared__ float red_v[8][BEAM_MAXK];
  __shared__ int red_i[8];
  __shared__ float top_v[2 * BEAM_MAXK];
  __shared__ int top_i[2 * BEAM_MAXK];
  __shared__ int n_parent[BEAM_MAXK], n_tok[BEAM_MAXK];
  __shared__ float n_score[BEAM_MAXK];
  __shared__ float n_lp[BEAM_MAXK], eos_lp[BEAM_MAXK];   // log-probability of each row's chosen token / of EOS after each row
  __shared__ float row_m[BEAM_MAXK], row_lse[BEAM_MAXK];
  __shared__ int was_done;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x, r0 = g * k;
  const int t = state[ST_T];                    // token step (beam mode has no prefix)
  int* rec = hyp + (size_t)g * BEAM_HREC;
  if (tid == 0) was_done = rec[2];
  __syncthreads();
  if (was_done) {
    // a finished group emits pad and keeps its rows (BeamSearchScorer.process pads a done group)
    if (tid < k) { n_parent[tid] = r0 + tid; n_tok[tid] = pad; n_score[tid] = 0.f; n_lp[tid] = 0.f; eos_lp[tid] = 0.f; }
  } else {
    const float* lg = logits + (size_t)r0 * V;
    // row max (NaN-propagating, as log_softmax of a row holding a NaN is NaN everywhere), then sum of exp
    float m[BEAM_MAXK], se[BEAM_MAXK];
#pragma unroll
    for (int j = 0; j < BEAM_MAXK; ++j) {
      m[j] = -INFINITY;
      if (j < k)
        for (int c = tid; c < V; c += 512) m[j] = nanmax(m[j], lg[(size_t)j * V + c]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m[j] = nanmax(m[j], __shfl_xor(m[j], off, 64));
      if (lane == 0) red_v[wave][j] = m[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BEAM_MAXK; ++j) {
      float mm = red_v[0][j];
#pragma unroll
      for (int w = 1; w < 8; ++w) mm = nanmax(mm, red_v[w][j]);
      m[j] = mm;
      se[j] = 0.f;
      if (j < k)
        for (int c = tid; c < V; c += 512) se[j] += expf(lg[(size_t)j * V + c] - mm);
      se[j] = wave_sum(se[j]);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < BEAM_MAXK; ++j) red_v[wave][j] = se[j];
    }
    __syncthreads();
    for (int j = 0; j < k; ++j) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) s += red_v[w][j];
      const float lse = logf(s), bs = bscore[r0 + j];
      if (tid == 0) { row_m[j] = m[j]; row_lse[j] = lse; }
      for (int c = tid; c < V; c += 512) {
        const float lp = (lg[(size_t)j * V + c] - m[j]) - lse;          // log_softmax, as torch computes it
        sc[j * V + c] = (ban != nullptr && ban[(size_t)(r0 + j) * ban_stride + c]) ? -INFINITY : lp + bs;
      }
    }
    __syncthreads();
    // top 2k, one per round
    const int n = k * V;
    float pv = 0.f;
    int pi = -1;
    for (int rnk = 0; rnk < 2 * k; ++rnk) {
      float bv = -INFINITY;
      int bi = -1;
      for (int c = tid; c < n; c += 512) {
        const float v = sc[c];
        if ((pi < 0 || argmax_beats(pv, pi, v, c)) && argmax_beats(v, c, bv, bi)) { bv = v; bi = c; }
      }
      rank_reduce_wave(bv, bi);
      if (lane == 0) { red_v[wave][0] = bv; red_i[wave] = bi; }
      __syncthreads();
      bv = red_v[0][0]; bi = red_i[0];
#pragma unroll
      for (int w = 1; w < 8; ++w)
        if (argmax_beats(red_v[w][0], red_i[w], bv, bi)) { bv = red_v[w][0]; bi = red_i[w]; }
      if (tid == 0) { top_v[rnk] = bv; top_i[rnk] = bi; }
      pv = bv; pi = bi;
      __syncthreads();
    }
    if (tid == 0) {
      // BeamSearchScorer.process: cur_len = 1 + t (start token included)
      const float denom = powf((float)(t + 1), length_penalty);
      int nb = 0;
      for (int rnk = 0; rnk < 2 * k && nb < k; ++rnk) {
        const int c = max(top_i[rnk], 0), j = c / V, tok = c - j * V;
        if (tok == eos) {
          if (rnk >= k) continue;                 // an EOS below the top k is not a hypothesis
          beam_hyp_add(rec, k, top_v[rnk] / denom, t, r0 + j);
        } else {
          n_parent[nb] = r0 + j; n_tok[nb] = tok; n_score[nb] = top_v[rnk];
          n_lp[nb] = (lg[(size_t)j * V + tok] - row_m[j]) - row_lse[j];      // the lp that went into sc, bit for bit
          ++nb;
        }
      }
      for (; nb < k; ++nb) { n_parent[nb] = r0 + nb; n_tok[nb] = pad; n_score[nb] = -INFINITY; n_lp[nb] = 0.f; }   // unreachable: <= k EOS
      for (int j = 0; j < k; ++j)
        eos_lp[j] = (eos < 0 || eos >= V) ? 0.f
                    : (ban != nullptr && ban[(size_t)(r0 + j) * ban_stride + eos]) ? -INFINITY
                                                                                   : (lg[(size_t)j * V + eos] - row_m[j]) - row_lse[j];
      // BeamHypotheses.is_done(best candidate score, cur_len), early_stopping = False
      if (rec[0] >= k && __int_as_float(rec[1]) >= top_v[0] / denom) rec[2] = 1;
    }
  }
  __syncthreads();
  const float* pr = pos + (size_t)(t + 1) * DMODEL;
  for (int j = 0; j < k; ++j) {
    const int row = r0 + j, tok = n_tok[j];
    x[(size_t)row * DMODEL + tid] = embed[(size_t)tok * DMODEL + tid] + pr[tid];      // 512 threads = DMODEL
  }
  if (tid < k) {
    const int row = r0 + tid;
    bscore[row] = n_score[tid];
    bp[((size_t)t * rows + row) * 2] = n_parent[tid];
    bp[((size_t)t * rows + row) * 2 + 1] = n_tok[tid];
    tokens[(size_t)row * tok_ld + t + 1] = n_tok[tid];
    // plane 0: lp of the token row `row` took at step t; plane 1: lp of EOS after the prefix row `row` held BEFORE step t
    blp[(size_t)t * rows + row] = n_lp[tid];
    blp[blp_plane + (size_t)t * rows + row] = eos_lp[tid];
  }
  __syncthreads();
  if (tid == 0) {
    if (rec[2])
      for (int j = 0; j < k; ++j) __hip_atomic_store(&state[ST_FLAGS + r0 + j], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    dec_step_close(state, rows, t, t, true);
  }
}

// KV-cache reorder after dec_beam_select: positions 0..t of every layer's self-attention K and V move from row
// parent(row) to row, for each row whose parent is another row.  No staging buffer: a parent is always in the row's own
// group, and one thread owns the same 16-byte slots of every row of a group, so it loads the source of every slot it
// will write into registers (<= 8 rows x 2 slots), waits for them, then stores: any parent map, swaps and
// one parent with several children included, is read before it is written.  Work item = (group, layer, K|V, 8 KB
// chunk of the live prefix); a fixed grid strides over the items that exist at this step (t is read on the device).
#define REORDER_THREADS 256
#define REORDER_U4 (2 * REORDER_THREADS)   // 16-byte slots per row per work item
__global__ __launch_bounds__(REORDER_THREADS) void dec_beam_reorder(char* __restrict__ kc, char* __restrict__ vc,
                                                                    size_t layer_bytes, size_t row_bytes, int pos_bytes,
                                                                    int n_layers, int groups, int k,
                                                                    const int* __restrict__ bp,
                                                                    const int* __restrict__ state) {
  const int t1 = state[ST_T];                   // the select kernel has advanced it: live positions 0..t1-1
  const int rows = groups * k;
  const size_t n16 = (size_t)t1 * pos_bytes / 16;
  const int chunks = (int)((n16 + REORDER_U4 - 1) / REORDER_U4);
  const int items = groups * 2 * n_layers * chunks;
  const int* par = bp + (size_t)(t1 - 1) * rows * 2;
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    const int ch = it % chunks, lk = (it / chunks) % (2 * n_layers), g = it / (chunks * 2 * n_layers);
    char* base = ((lk & 1) ? vc : kc) + (size_t)(lk >> 1) * layer_bytes;
    int pj[BEAM_MAXK];
    bool any = false;
#pragma unroll
    for (int j = 0; j < BEAM_MAXK; ++j) {
      pj[j] = (j < k) ? par[(size_t)(g * k + j) * 2] : g * k + j;
      any |= pj[j] != g * k + j;
    }
    if (!any) continue;
    u32x4 buf[BEAM_MAXK][2];
#pragma unroll
    for (int j = 0; j < BEAM_MAXK; ++j)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const size_t e = (size_t)ch * REORDER_U4 + u * REORDER_THREADS + threadIdx.x;
        if (pj[j] != g * k + j && e < n16) buf[j][u] = ((const u32x4*)(base + (size_t)pj[j] * row_bytes))[e];
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < BEAM_MAXK; ++j)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const size_t e = (size_t)ch * REORDER_U4 + u * REORDER_THREADS + threadIdx.x;
        if (pj[j] != g * k + j && e < n16) ((u32x4*)(base + (size_t)(g * k + j) * row_bytes))[e] = buf[j][u];
      }
  }
}

// Beam scores [0, -1e9, ...] per group, empty hypothesis records.
__global__ void dec_beam_begin_kernel(int groups, int k, float* bscore, int* hyp) {
  for (int i = threadIdx.x; i < groups * k; i += blockDim.x) bscore[i] = (i % k == 0) ? 0.f : -1e9f;
  for (int g = threadIdx.x; g < groups; g += blockDim.x) {
    int* rec = hyp + (size_t)g * BEAM_HREC;
    rec[0] = 0; rec[1] = __float_as_int(1e9f); rec[2] = 0; rec[3] = 0;
  }
}

// BeamSearchScorer.finalize: the running beams of a group that is not done become hypotheses (length 1 + T, T = steps
// run), the best one (the last added of equal best scores: stable sort + pop) is read back through the backpointers
// into out[g] = start, tokens..., EOS when shorter than 1 + max_length, pad to ld.  One thread per group.
__global__ void dec_beam_finalize_kernel(int groups, int k, int rows, const int* __restrict__ state,
                                        const float* __restrict__ bscore, const int* __restrict__ bp, int* __restrict__ hyp,
                                        float length_penalty, int64_t* __restrict__ out, int ld, int max_length,
                                        int start, int eos, int pad, const float* __restrict__ blp, size_t blp_plane,
                                        float* __restrict__ out_logp) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= groups) return;
  int* rec = hyp + (size_t)g * BEAM_HREC;
  const int T = state[ST_T];
  if (!rec[2]) {
    const float denom = powf((float)(T + 1), length_penalty);
    for (int j = 0; j < k; ++j) beam_hyp_add(rec, k, bscore[g * k + j] / denom, T, g * k + j);
  }
  int best = 0;
  for (int i = 1; i < rec[0]; ++i)
    if (__int_as_float(rec[BEAM_HYP0 + 3 * i]) >= __int_as_float(rec[BEAM_HYP0 + 3 * best])) best = i;
  const int end = rec[BEAM_HYP0 + 3 * best + 1];
  const int e = min(end, max_length);
  int r = rec[BEAM_HYP0 + 3 * best + 2];
  int64_t* o = out + (size_t)g * ld;
  float* ol = out_logp ? out_logp + (size_t)g * ld : nullptr;
  const int len = 1 + e;
  if (ol) {
    // the closing EOS: a hypothesis that ended at a step (end < T) took EOS after row r's prefix at that step; one
    // that is a running beam (end = T) has none to score
    ol[0] = 0.f;
    for (int c = len; c < ld; ++c) ol[c] = (c == len && len < 1 + max_length && end < T) ? blp[blp_plane + (size_t)end * rows + r] : 0.f;
  }
  o[0] = start;
  for (int s = e - 1; s >= 0; --s) {
    const int* b = bp + ((size_t)s * rows + r) * 2;
    o[s + 1] = b[1];
    if (ol) ol[s + 1] = blp[(size_t)s * rows + r];
    r = b[0];
  }
  for (int c = len; c < ld; ++c) o[c] = (c == len && len < 1 + max_length) ? eos : pad;
  rec[3] = len;
}

extern "C" int mrmt3_decoder_set_ban(mrmt3_decoder* D, const uint8_t* banned_mask, void* stream) {
  (void)stream;
  MR_CHECK_ARG(D && D->tokens, "decoder_set_ban: call decoder_begin first");
  MR_CHECK_ARG(D->tail.k == 0, "decoder_set_ban: beam mode takes its mask in decoder_begin_beam");
  MR_CHECK_ARG(!D->tail.gram, "decoder_set_ban: call it before decoder_set_grammar (the grammar's masks take the ban in)");
  D->tail.ban = banned_mask;
  return MRMT3_OK;
}

// column 0 (the start token) of the log-probability rows
__global__ void dec_logp_begin_kernel(int B, float* logp, int ld) {
  for (int b = threadIdx.x; b < B; b += blockDim.x) logp[(size_t)b * ld] = 0.f;
}

extern "C" int mrmt3_decoder_set_logprobs(mrmt3_decoder* D, float* out, int ld, void* stream) {
  MR_CHECK_ARG(D && D->tokens, "decoder_set_logprobs: call decoder_begin first");
  MR_CHECK_ARG(D->tail.k == 0, "decoder_set_logprobs: beam mode returns them from decoder_beam_finalize_logprobs");
  if (!out) { D->tail.logp = nullptr; D->tail.logp_ld = 0; return MRMT3_OK; }
  MR_CHECK_ARG(ld >= D->maxLen + 1, "decoder_set_logprobs: need ld >= max_len + 1 (%d), got %d", D->maxLen + 1, ld);
  MR_CHECK_ARG(D->V <= 64 * LOGP_REGS, "decoder_set_logprobs: vocab %d exceeds the %d logits a wave keeps in registers",
               D->V, 64 * LOGP_REGS);
  D->tail.logp = out; D->tail.logp_ld = ld;
  hipLaunchKernelGGL(dec_logp_begin_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, D->B, out, ld);
  MR_CHECK_LAUNCH("decoder_set_logprobs");
  return MRMT3_OK;
}

static int sample_check_args(const char* who, float temperature, int top_k, float top_p, int V) {
  MR_CHECK_ARG(temperature > 0.f && temperature <= 3.0e38f, "%s: need a finite temperature > 0, got %g", who, (double)temperature);
  MR_CHECK_ARG(top_k >= 0, "%s: need top_k >= 0 (0 = off), got %d", who, top_k);
  MR_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "%s: need top_p in (0, 1], got %g", who, (double)top_p);
  MR_CHECK_ARG(V <= 64 * LOGP_REGS, "%s: vocab %d exceeds the %d logits a wave keeps in registers", who, V, 64 * LOGP_REGS);
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_set_sampling(mrmt3_decoder* D, float temperature, int top_k, float top_p,
                                          unsigned long long seed, void* stream) {
  MR_CHECK_ARG(D && D->tokens, "decoder_set_sampling: call decoder_begin first");
  if (temperature == 0.f) { D->tail.sample = 0; return MRMT3_OK; }      // back to the greedy tail
  MR_CHECK_ARG(D->tail.k == 0, "decoder_set_sampling: beam search does not sample");
  int rc = sample_check_args("decoder_set_sampling", temperature, top_k, top_p, D->V);
  if (rc != MRMT3_OK) return rc;
  const SampleCfg c = {temperature, top_k, top_p, sample_seed_key(seed)};
  hipLaunchKernelGGL(dec_sampling_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, D->samp, c);
  MR_CHECK_LAUNCH("decoder_set_sampling");
  D->tail.sample = 1;
  return MRMT3_OK;
}

extern "C" int mrmt3_sample_logits(const float* logits, int rows, int V, const uint8_t* banned_mask, float temperature,
                                   int top_k, float top_p, unsigned long long seed, int step, int row0,
                                   int64_t* tokens_out, float* logp_out, void* stream) {
  MR_CHECK_ARG(logits && tokens_out && rows > 0 && V > 0 && step >= 0 && row0 >= 0, "sample_logits: bad args");
  int rc = sample_check_args("sample_logits", temperature, top_k, top_p, V);
  if (rc != MRMT3_OK) return rc;
  const SampleCfg c = {temperature, top_k, top_p, sample_seed_key(seed)};
  const dim3 grid((unsigned)ceil_div(rows, 8)), block(512);
#define SAMPLE_LOGITS(BAN, LOGP)                                                                                      \
  hipLaunchKernelGGL((sample_logits_kernel<BAN, LOGP>), grid, block, 0, (hipStream_t)stream, logits, rows, V, banned_mask, \
                     c, (unsigned)step, (unsigned)row0, tokens_out, logp_out)
  if (logp_out) { if (banned_mask) SAMPLE_LOGITS(true, true); else SAMPLE_LOGITS(false, true); }
  else if (banned_mask) SAMPLE_LOGITS(true, false);
  else SAMPLE_LOGITS(false, false);
#undef SAMPLE_LOGITS
  MR_CHECK_LAUNCH("sample_logits");
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_begin_beam(mrmt3_decoder* D, const mrmt3_decoder_weights* w, const void* cross_kv, int groups,
                                        int num_beams, int enc_len, int64_t* tokens_out, int start_id, int eos_id,
                                        int pad_id, float length_penalty, const uint8_t* banned_mask, int32_t* backptr,
                                        float* beam_scores, int32_t* hyps, void* stream) {
  MR_CHECK_ARG(D && w && cross_kv && tokens_out && backptr && beam_scores && hyps, "decoder_begin_beam: null pointer");
  MR_CHECK_ARG(num_beams >= 1 && num_beams <= BEAM_MAXK, "decoder_begin_beam: need 1 <= num_beams <= 8, got %d", num_beams);
  MR_CHECK_ARG(groups > 0 && (long)groups * num_beams <= D->maxB, "decoder_begin_beam: groups x num_beams (%d x %d) exceeds max_batch %d",
               groups, num_beams, D->maxB);
  MR_CHECK_ARG(D->V >= 2 && (size_t)num_beams * D->V * sizeof(float) <= 65536,
               "decoder_begin_beam: num_beams x vocab scores must fit 64 KiB of LDS");
  MR_CHECK_ARG(D->n_prefix == 0, "decoder_begin_beam: a prefix is set on the handle");
  int rc = mrmt3_decoder_begin(D, w, cross_kv, groups * num_beams, enc_len, tokens_out, start_id, eos_id, pad_id, stream);
  if (rc != MRMT3_OK) return rc;
  D->tail.k = num_beams; D->tail.groups = groups; D->tail.length_penalty = length_penalty; D->tail.ban = banned_mask;
  D->tail.bscore = beam_scores; D->tail.bp = backptr; D->tail.hyp = hyps;
  hipLaunchKernelGGL(dec_beam_begin_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, groups, num_beams, beam_scores, hyps);
  MR_CHECK_LAUNCH("decoder_begin_beam");
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_beam_finalize(mrmt3_decoder* D, int64_t* out_ids, int ld, int max_length, void* stream) {
  return mrmt3_decoder_beam_finalize_logprobs(D, out_ids, nullptr, ld, max_length, stream);
}

extern "C" int mrmt3_decoder_beam_finalize_logprobs(mrmt3_decoder* D, int64_t* out_ids, float* out_logp, int ld,
                                                    int max_length, void* stream) {
  MR_CHECK_ARG(D && out_ids, "decoder_beam_finalize: null pointer");
  MR_CHECK_ARG(D->tokens && D->tail.k > 0, "decoder_beam_finalize: call decoder_begin_beam first");
  MR_CHECK_ARG(max_length >= 0 && max_length <= D->maxLen && ld >= 1 + max_length,
               "decoder_beam_finalize: need 0 <= max_length <= max_len and ld >= 1 + max_length");
  const mrmt3_decoder::Tail& T = D->tail;
  D->beam_out = out_ids; D->beam_out_ld = ld; D->beam_out_len = max_length;
  hipLaunchKernelGGL(dec_beam_finalize_kernel, dim3((unsigned)ceil_div(T.groups, 64)), dim3(64), 0, (hipStream_t)stream,
                     T.groups, T.k, D->B, (const int*)D->state, (const float*)T.bscore, (const int*)T.bp, T.hyp,
                     T.length_penalty, out_ids, ld, max_length, D->start, D->eos, D->pad, (const float*)D->blp,
                     (size_t)D->maxLen * D->maxB, out_logp);
  MR_CHECK_LAUNCH("decoder_beam_finalize");
  return MRMT3_OK;
}

// the step's last kernel(s): greedy argmax (banned or not), the sampled tail, or the beam select + KV-cache reorder
void mrmt3_dec_launch_tail(mrmt3_decoder* D, hipStream_t s) {
  const int B = D->B, V = D->V;
  if (D->tail.k > 0) {
    const mrmt3_decoder::Tail& T = D->tail;
    hipLaunchKernelGGL(dec_beam_select, dim3((unsigned)T.groups), dim3(512), (size_t)T.k * V * sizeof(float), s, D->logits,
                       V, T.k, B, D->tokens, D->maxLen + 1, (const float*)D->w.embed, D->w.pos, D->x, D->state, D->eos,
                       D->pad, T.length_penalty, T.ban, T.bscore, T.bp, T.hyp, D->blp, (size_t)D->maxLen * D->maxB,
                       T.ban_stride);
    const size_t esz = D->wdt == MRMT3_BF16 ? 2 : 4;
    const size_t row_bytes = (size_t)D->maxLen * D->inner * esz, layer_bytes = (size_t)D->maxB * row_bytes;
    const size_t max_items = (size_t)T.groups * 2 * D->L * ceil_div((int)(row_bytes / 16), REORDER_U4);
    hipLaunchKernelGGL(dec_beam_reorder, dim3((unsigned)std::min<size_t>(max_items, 2048)), dim3(REORDER_THREADS), 0, s,
                       (char*)D->kc, (char*)D->vc, layer_bytes, row_bytes, (int)(D->inner * esz), D->L, T.groups, T.k,
                       (const int*)T.bp, (const int*)D->state);
  } else {
    // the argument list dec_argmax and dec_sample share; `more`: what dec_sample takes beyond it
    auto launch = [&](auto kernel, auto... more) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(B, 8)), dim3(512), 0, s, D->logits, V, B, D->tokens, D->maxLen + 1,
                         (const float*)D->w.embed, D->w.pos, D->x, D->state, D->eos, D->pad, D->prefix, D->tail.ban,
                         D->tail.logp, D->tail.logp_ld, more...);
    };
    auto tail = [&](auto ban, auto lp) {
      if (D->tail.sample) launch(dec_sample<ban.value, lp.value>, (const SampleCfg*)D->samp, D->tail.ban_stride);
      else launch(dec_argmax<ban.value, lp.value>, D->tail.ban_stride);
    };
    auto with_lp = [&](auto ban) { D->tail.logp ? tail(ban, std::true_type{}) : tail(ban, std::false_type{}); };
    D->tail.ban ? with_lp(std::true_type{}) : with_lp(std::false_type{});
  }
  if (D->tail.gram) mrmt3_dec_launch_grammar_step(D, s);
}
