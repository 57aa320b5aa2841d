// K12 — greedy autoregressive decode with a self-attention KV cache, one hipGraph replay per token.
//
// Stands for the decoder loop of models/t5.py:267-295 (batched, MT3Net) and
// models/t5_segmem_v2_with_prev.py:273-291 (one segment at a time).  The reference re-runs the
// whole decoder over the growing prefix for every token (no cache, O(L^2) GEMM work) and, in the
// segment-memory model, synchronises with the host once per token (`.item()`, :284).  Here a step
// is 66 small kernels captured once into a hipGraph:
//   per layer  norm+QKV gemv (K/V appended to the cache) -> self-attention over the cache ->
//              O gemv + residual -> norm+Q gemv -> cross-attention over the projected encoder
//              states -> O gemv + residual -> norm + wi gemv + gated-GELU -> wo gemv + residual
//   then       final norm + lm_head gemv -> argmax / EOS bookkeeping / next-token embedding.
// The step index and the finished flags live in device memory, so replays need no host
// interaction; the host polls an 12-byte status block only when it wants to stop early.
// A step is a chain of dependent launches (1.77 us each at best on this runtime), so every kernel is built to be
// short rather than frugal: up to 8 sequences run one weight row x one sequence per wave (batch on gridDim.y;
// the re-read of a weight row by the other sequences is an L2 hit), larger batches (<= 256) multiply 16 rows by
// 16 sequences on the matrix cores with K split over a workgroup; the 45.6 MB (bf16) of per-step weights stay
// resident in the 256 MB Infinity Cache.  mrmt3_decoder_set_prefix feeds memory rows before the start token
// (the V1 segment-memory decode).  mrmt3_decoder_set_ban / mrmt3_decoder_begin_beam swap the step's tail for a masked
// argmax or for beam search (select + KV-cache reorder), mrmt3_decoder_set_sampling for a draw from the
// filtered distribution; the 65 kernels before it are shared.  mrmt3_decoder_set_grammar appends dec_grammar_step:
// the MT3 event grammar per row, whose allowed set is the next step's ban mask, one row per decode row.
#include "common.h"

#define DMODEL 512
#define DEC_MAXB 256
#ifndef DEC_MFMA_ABOVE
#define DEC_MFMA_ABOVE 8   // batches larger than this use the 16-sequence MFMA projections (bf16 weights)
#endif
#define ST_CNT (ST_FLAGS + DEC_MAXB)   // workgroups of the current argmax launch that have finished

template <typename T> __device__ __forceinline__ void load8(const T* p, float v[8]);
template <> __device__ __forceinline__ void load8<float>(const float* p, float v[8]) {
  f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float v[8]) {
  u32x4 t = *(const u32x4*)p;
  v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xFFFF0000u);
  v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xFFFF0000u);
  v[4] = __uint_as_float(t.z << 16); v[5] = __uint_as_float(t.z & 0xFFFF0000u);
  v[6] = __uint_as_float(t.w << 16); v[7] = __uint_as_float(t.w & 0xFFFF0000u);
}
// activations entering a projection are rounded to the weights' dtype, as in the engine's bf16 GEMMs
// (identity for the fp32 parity path)
template <typename TW> __device__ __forceinline__ float act_round(float v);
template <> __device__ __forceinline__ float act_round<float>(float v) { return v; }
template <> __device__ __forceinline__ float act_round<bf16_t>(float v) { return bf2f(f2bf(v)); }
template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <typename T> __device__ __forceinline__ void stf(T* p, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void stf<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }

__device__ __forceinline__ float gelu_new_d(float x) {
  const float c = 0.7978845608028654f;
  return 0.5f * x * (1.0f + tanhf(c * (x + 0.044715f * (x * x * x))));
}

// state block: [0] step t, [1] all finished, [2] step at which the last row finished (-1), [4+b] finished[b]
#define ST_T 0
#define ST_ALL 1
#define ST_FIN 2
#define ST_NPRE 3   // number of prefix (memory) positions fed before the start token
#define ST_FLAGS 4

// ---- norm + gemv -------------------------------------------------------------------------------------
// One wave = one weight row (two for the gated FFN) x ONE sequence; the batch is gridDim.y.  Measured on
// MI355X: a decode step is a chain of ~66 dependent launches whose length is set by the slowest wave of
// each, so the lightest possible wave wins — carrying 2 rows or up to 8 sequences per wave (to stream a
// weight row once) cost 255 / 607 us per step at batch 1 / 8 against 235 / 277 this way; the re-read of
// a weight row by the other sequences' waves is an L2 hit.
// Every wave normalises x[b] for itself from registers (8 elements per lane, one wave_sum) — no LDS, no
// workgroup barrier — and requests its weight row before anything else.
// MODE 0: out[b][n] (f32, ld = N)      — cross-attention q, lm_head logits
// MODE 1: fused q|k|v: n < inner -> q scratch; else K / V cache row t of this layer
// MODE 2: gated GELU: rows n and n+N of W ([2N][512]) -> out[b][n] = gelu_new(h0) * h1
#ifndef DEC_WPG
#define DEC_WPG 4   // waves (rows) per workgroup
#endif
template <typename TW, int MODE>
__global__ __launch_bounds__(64 * DEC_WPG) void dec_norm_gemv(const float* __restrict__ x, const float* __restrict__ lnw,
                                                             const TW* __restrict__ W, int N, float eps,
                                                             float* __restrict__ out, TW* __restrict__ kc,
                                                             TW* __restrict__ vc, int inner, size_t cache_bstride,
                                                             const int* __restrict__ state) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * DEC_WPG + wave, b = blockIdx.y;
  if (n >= N) return;
  float w0[8], w1[8], lw[8], xn[8];
  load8<TW>(W + (size_t)n * DMODEL + lane * 8, w0);
  if (MODE == 2) load8<TW>(W + (size_t)(n + N) * DMODEL + lane * 8, w1);
  load8<float>(lnw + lane * 8, lw);
  load8<float>(x + (size_t)b * DMODEL + lane * 8, xn);
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) ss = fmaf(xn[e], xn[e], ss);
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / (float)DMODEL + eps);
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = act_round<TW>(lw[e] * (xn[e] * rstd));
    s0 = fmaf(w0[e], v, s0);
    if (MODE == 2) s1 = fmaf(w1[e], v, s1);
  }
  s0 = wave_sum(s0);
  if (MODE == 2) s1 = wave_sum(s1);
  if (lane == 0) {
    if (MODE == 0) out[(size_t)b * N + n] = s0;
    else if (MODE == 2) out[(size_t)b * N + n] = gelu_new_d(s0) * s1;
    else {
      const int t = state[ST_T];
      if (n < inner) out[(size_t)b * inner + n] = s0;
      else if (n < 2 * inner) stf<TW>(kc + b * cache_bstride + (size_t)t * inner + (n - inner), s0);
      else stf<TW>(vc + b * cache_bstride + (size_t)t * inner + (n - 2 * inner), s0);
    }
  }
}

// x[b][n] += sum_k a[b][k] * W[n][k]   (O projections and FFN wo, residual add fused); K <= 1024.
// Weight row, activation vector and the residual value to update are all requested up front.
template <typename TW, int KCH>   // KCH = number of 512-element chunks of K (1 or 2)
__global__ __launch_bounds__(64 * DEC_WPG) void dec_gemv_res(const float* __restrict__ a, const TW* __restrict__ W,
                                                            float* __restrict__ x, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * DEC_WPG + wave, b = blockIdx.y;
  if (n >= N) return;
  float w[KCH][8], av[KCH][8];
#pragma unroll
  for (int c = 0; c < KCH; ++c) {
    const int k0 = c * 512 + lane * 8;
    if (k0 < K) {
      load8<TW>(W + (size_t)n * K + k0, w[c]);
      load8<float>(a + (size_t)b * K + k0, av[c]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) { w[c][e] = 0.f; av[c][e] = 0.f; }
    }
  }
  float* xdst = x + (size_t)b * N + n;
  const float xold = (lane == 0) ? *xdst : 0.f;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < KCH; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(w[c][e], act_round<TW>(av[c][e]), acc);
  acc = wave_sum(acc);
  if (lane == 0) *xdst = xold + acc;
}

// ---- the same two projections for groups of 16 sequences on the matrix cores (bf16 weights, batch > 8) ----
// With one sequence per wave every sequence re-reads every weight row from L2 (45.6 MB x B per step: at 64
// sequences that, not the launch chain, set the step time).  Here a wave multiplies 16 weight rows by 16
// sequences: D[16 rows][16 seq] = W[16][K] . A^T[K][16] as K/32 v_mfma_f32_16x16x32_bf16, operands loaded
// straight from global memory in fragment layout (lane = (row or sequence) & 15, k-group = lane >> 4 holds
// 8 consecutive k).  Same operand precision and the same products as the single-sequence kernels above; only
// the order of the f32 additions differs.
__device__ __forceinline__ bf16x8 pack8(const float v[8]) {
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (short)f2bf(v[e]);
  return r;
}

// A workgroup = 16 weight rows x 16 sequences; its 4 waves split K (a projection has only 384-2048 rows, so
// 16 rows per WAVE would leave most CUs idle and make each busy one pull hundreds of KB), partial tiles are
// summed through LDS in wave order.
template <int MODE>
__global__ __launch_bounds__(256) void dec_norm_gemm16(const float* __restrict__ x, const float* __restrict__ lnw,
                                                       const bf16_t* __restrict__ W, int N, float eps,
                                                       float* __restrict__ out, bf16_t* __restrict__ kc,
                                                       bf16_t* __restrict__ vc, int inner, size_t cache_bstride,
                                                       const int* __restrict__ state, int B) {
  constexpr int KB = DMODEL / 32 / 4;          // k-blocks of 32 per wave
  __shared__ float ssq[4][16];
  __shared__ float part[2][4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int seq = blockIdx.y * 16 + r;
  const int k0 = wave * (DMODEL / 4) + g * 8;   // this lane's first k
  const bf16_t* wrow = W + (size_t)min(n0 + r, N - 1) * DMODEL + k0;
  bf16x8 a0[KB], a1[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    a0[kb] = *(const bf16x8*)(wrow + kb * 32);
    if (MODE == 2) a1[kb] = *(const bf16x8*)(wrow + (size_t)N * DMODEL + kb * 32);
  }
  const float* xs = x + (size_t)min(seq, B - 1) * DMODEL + k0;
  float xv[KB][8], lw[KB][8];
  float ss = 0.f;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    load8<float>(xs + kb * 32, xv[kb]);
    load8<float>(lnw + k0 + kb * 32, lw[kb]);
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(xv[kb][e], xv[kb][e], ss);
  }
  ss += __shfl_xor(ss, 16, 64);
  ss += __shfl_xor(ss, 32, 64);
  if (g == 0) ssq[wave][r] = ss;
  __syncthreads();
  const float rstd = rsqrtf(((ssq[0][r] + ssq[1][r]) + (ssq[2][r] + ssq[3][r])) / (float)DMODEL + eps);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = lw[kb][e] * (xv[kb][e] * rstd);
    const bf16x8 bfr = pack8(v);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[kb], bfr, acc0, 0, 0, 0);
    if (MODE == 2) acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[kb], bfr, acc1, 0, 0, 0);
  }
  // D: column = lane & 15 = sequence, rows 4 g + (0..3); element id = (4 g + rr) * 16 + r
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    part[0][wave][(g * 4 + rr) * 16 + r] = acc0[rr];
    if (MODE == 2) part[1][wave][(g * 4 + rr) * 16 + r] = acc1[rr];
  }
  __syncthreads();
  const int id = threadIdx.x;                   // one output element per thread: row id / 16, sequence id % 16
  const int n = n0 + (id >> 4), sq = blockIdx.y * 16 + (id & 15);
  if (n >= N || sq >= B) return;
  const float s0 = (part[0][0][id] + part[0][1][id]) + (part[0][2][id] + part[0][3][id]);
  if (MODE == 0) out[(size_t)sq * N + n] = s0;
  else if (MODE == 2)
    out[(size_t)sq * N + n] = gelu_new_d(s0) * ((part[1][0][id] + part[1][1][id]) + (part[1][2][id] + part[1][3][id]));
  else {
    const int t = state[ST_T];
    if (n < inner) out[(size_t)sq * inner + n] = s0;
    else if (n < 2 * inner) kc[sq * cache_bstride + (size_t)t * inner + (n - inner)] = f2bf(s0);
    else vc[sq * cache_bstride + (size_t)t * inner + (n - 2 * inner)] = f2bf(s0);
  }
}

template <int KB>   // K / 32 / 4 : k-blocks per wave
__global__ __launch_bounds__(256) void dec_gemm16_res(const float* __restrict__ a, const bf16_t* __restrict__ W,
                                                      float* __restrict__ x, int N, int B) {
  constexpr int K = KB * 32 * 4;
  __shared__ float part[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int seq = blockIdx.y * 16 + r;
  const int k0 = wave * (K / 4) + g * 8;
  const bf16_t* wrow = W + (size_t)min(n0 + r, N - 1) * K + k0;
  const float* as = a + (size_t)min(seq, B - 1) * K + k0;
  const int id = threadIdx.x;
  const int n = n0 + (id >> 4), sq = blockIdx.y * 16 + (id & 15);
  const bool live = n < N && sq < B;
  const float xold = live ? x[(size_t)sq * N + n] : 0.f;
  bf16x8 wf[KB];
  float av[KB][8];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    wf[kb] = *(const bf16x8*)(wrow + kb * 32);
    load8<float>(as + kb * 32, av[kb]);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[kb], pack8(av[kb]), acc, 0, 0, 0);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) part[wave][(g * 4 + rr) * 16 + r] = acc[rr];
  __syncthreads();
  if (live) x[(size_t)sq * N + n] = xold + ((part[0][id] + part[1][id]) + (part[2][id] + part[3][id]));
}

// one (head, batch) per workgroup: softmax(q.K^T) V over `len` cached rows (len = t+1 or fixed).
// The kernel is a chain of L2 round trips, so every phase issues all the loads it can before it waits:
// scores: one key per thread (8 x 16-byte loads of the key row), the first batch requested before q is
// staged and each later batch requested before the previous one is consumed.  PV: thread = (32 key
// lanes) x (8 dim-groups of 8), eight predicated 16-byte V loads in flight per thread, 32 independent
// partial sums reduced through LDS.
// (Computing the cross-attention query inside this kernel, 16 rows per wave while the key rows are in
// flight, saved a launch per layer and cost the same time: reverted.)
template <typename TC>
__global__ __launch_bounds__(256) void dec_attn(const float* __restrict__ q, const TC* __restrict__ kb,
                                                const TC* __restrict__ vb, int ld, size_t bstride, int fixed_len,
                                                const int* __restrict__ state, float* __restrict__ o, int inner) {
  extern __shared__ __attribute__((aligned(16))) float sm[];  // scores[len] | q[64] | red[8] | part[32][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, b = blockIdx.y;
  const int len = fixed_len > 0 ? fixed_len : state[ST_T] + 1;
  float* sc = sm;
  float* qs = sm + ((len + 3) & ~3);
  float* red = qs + 64;
  float* part = red + 8;
  const TC* kp = kb + b * bstride + h * 64;
  const TC* vp = vb + b * bstride + h * 64;
  const int nb = (len + 255) >> 8;            // key batches of 256 (block-uniform)
  float kva[8][8], kvb[8][8];
  auto fetch = [&](float (&dst)[8][8], int key) {
    const TC* kr = kp + (size_t)min(key, len - 1) * ld;
#pragma unroll
    for (int d0 = 0; d0 < 8; ++d0) load8<TC>(kr + d0 * 8, dst[d0]);
  };
  fetch(kva, tid);
  if (tid < 64) qs[tid] = q[(size_t)b * inner + h * 64 + tid];
  __syncthreads();
  float mx = -INFINITY;
  auto score = [&](const float (&src)[8][8], int key) {
    float s = 0.f;
#pragma unroll
    for (int d0 = 0; d0 < 8; ++d0)
#pragma unroll
      for (int e = 0; e < 8; ++e) s = fmaf(qs[d0 * 8 + e], src[d0][e], s);
    if (key < len) {
      sc[key] = s;
      mx = fmaxf(mx, s);
    }
  };
  for (int it = 0; it < nb; it += 2) {
    const int key = it * 256 + tid;
    if (it + 1 < nb) fetch(kvb, key + 256);
    score(kva, key);
    if (it + 1 < nb) {
      if (it + 2 < nb) fetch(kva, key + 512);
      score(kvb, key + 256);
    }
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  // V rows of the first PV batch are requested before the exponentials (requesting them at kernel entry,
  // next to the first key batch, measured the same)
  const int dg = tid & 7, kl = tid >> 3;   // 8 dims per thread, 32 key lanes
  float vv[8][8];
#pragma unroll
  for (int u = 0; u < 8; ++u) load8<TC>(vp + (size_t)min(kl + 32 * u, len - 1) * ld + dg * 8, vv[u]);
  float se = 0.f;
  for (int key = tid; key < len; key += 256) {
    const float p = expf(sc[key] - mx);
    sc[key] = p;
    se += p;
  }
  se = wave_sum(se);
  if (lane == 0) red[4 + wave] = se;
  __syncthreads();
  se = (red[4] + red[5]) + (red[6] + red[7]);
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int k0 = kl; k0 < len; k0 += 256) {
    float pr[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) pr[u] = (k0 + 32 * u < len) ? sc[k0 + 32 * u] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(pr[u], vv[u][e], acc[e]);
    if (k0 + 256 < len) {
#pragma unroll
      for (int u = 0; u < 8; ++u) load8<TC>(vp + (size_t)min(k0 + 256 + 32 * u, len - 1) * ld + dg * 8, vv[u]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[kl * 64 + dg * 8 + e] = acc[e];
  __syncthreads();
  if (tid < 64) {
    float r = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) r += part[k * 64 + tid];
    o[(size_t)b * inner + h * 64 + tid] = r / se;
  }
}

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

// ---- a vocabulary row in one wave's registers (LOGP_REGS values per lane, V <= 64 * LOGP_REGS): rl[i] = column lane + 64 i
#define LOGP_REGS 32
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
struct SampleCfg {
  float temperature;   // > 0; 1 leaves the logits' bits alone
  int top_k;           // 0 = off
  float top_p;         // 1 = off, else in (0, 1)
  unsigned key;        // the seed folded to 32 bits (sample_seed_key)
};
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

// ---- event grammar: per-row state machine whose allowed set is the next step's ban mask ---------------
// A row's state: the scalars below and `active`, a 128 x 128 bit set over (program, pitch) — in the tie section the
// pairs declared so far, in the body the notes sounding.  Two copies per row: at token step t every row reads its
// parent's state from copy t & 1 and writes its own to copy (t + 1) & 1, so beam reparenting needs no ordering between
// rows.  One wave per row: lane l carries words 8 l .. 8 l + 7 of the set from the parent's copy to the row's own (the
// 2 KB copy is what reparenting costs), the lane that owns the touched word edits it on the way, and only the 128-bit
// slice of the program in force enters the mask.
#define GRAM_WORDS 512        // 128 * 128 / 32
#define GRAM_TIE 0
#define GRAM_BODY 1
#define GRAM_VEL_UNSET 0
#define GRAM_VEL_OFF 1
#define GRAM_VEL_ON 2
struct GramS { int mode, program, velocity, cur, acc; };     // program -1 = unset; cur, acc in steps
struct GramRow { GramS s; int _r[3]; unsigned active[GRAM_WORDS]; };   // 32 + 2048 bytes
struct GramHdr { int parity; int _r[3]; const uint8_t* carry; const uint8_t* ban; };   // stand-alone state: which copy is current
static_assert(sizeof(GramRow) == 32 + 4 * GRAM_WORDS && sizeof(GramHdr) == 32, "grammar state layout");
#define GRAM_OP_NONE 0
#define GRAM_OP_SET 1
#define GRAM_OP_CLEAR 2

// Push one token: the scalars change here, the bit operation on `active` (bit `idx`) is returned.  A token the
// grammar does not allow in this state changes nothing it should not: the masks keep such tokens from being emitted.
__device__ __forceinline__ int gram_push(const mrmt3_grammar& g, GramS& s, int tok, int& idx) {
  idx = 0;
  unsigned v = (unsigned)(tok - g.shift0);
  if (v < (unsigned)g.n_shift) {
    if (s.mode == GRAM_BODY) s.acc += (int)v;
    return GRAM_OP_NONE;
  }
  if (s.mode == GRAM_TIE) {
    if (tok == g.tie) s.mode = GRAM_BODY;
    else if ((v = (unsigned)(tok - g.program0)) < (unsigned)g.n_program) s.program = (int)v;
    else if ((v = (unsigned)(tok - g.pitch0)) < (unsigned)g.n_pitch && s.program >= 0) {
      idx = s.program * 128 + (int)v;
      return GRAM_OP_SET;
    }
    return GRAM_OP_NONE;
  }
  // any non-shift token in the body closes the shift run: decode_events restarts its step count there
  s.cur = max(s.cur, s.acc);
  s.acc = 0;
  if ((v = (unsigned)(tok - g.program0)) < (unsigned)g.n_program) s.program = (int)v;
  else if ((v = (unsigned)(tok - g.velocity0)) < (unsigned)g.n_velocity) s.velocity = v ? GRAM_VEL_ON : GRAM_VEL_OFF;
  else if ((v = (unsigned)(tok - g.pitch0)) < (unsigned)g.n_pitch && s.program >= 0 && s.velocity != GRAM_VEL_UNSET) {
    idx = s.program * 128 + (int)v;
    return s.velocity == GRAM_VEL_ON ? GRAM_OP_SET : GRAM_OP_CLEAR;
  }
  return GRAM_OP_NONE;
}

// Is token `col` allowed in state s?  act / car: the 128-bit slices of `active` / the carry for s.program (zeros when unset).
__device__ __forceinline__ bool gram_allowed(const mrmt3_grammar& g, const GramS& s, const unsigned (&act)[4],
                                             const unsigned (&car)[4], bool has_carry, int col) {
  const bool body = s.mode == GRAM_BODY;
  if (col == g.eos) return body;
  if (col == g.tie) return !body;
  unsigned v = (unsigned)(col - g.shift0);
  if (v < (unsigned)g.n_shift) return body && v >= 1u && s.cur < s.acc + (int)v && s.acc + (int)v <= g.max_shift_steps;
  if ((v = (unsigned)(col - g.pitch0)) < (unsigned)g.n_pitch) {
    if (s.program < 0) return false;
    unsigned aw = act[0], cw = car[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if ((v >> 5) == (unsigned)j) { aw = act[j]; cw = car[j]; }
    const bool on = (aw >> (v & 31u)) & 1u, carried = (cw >> (v & 31u)) & 1u;
    if (!body) return !on && (!has_carry || carried);
    return s.velocity == GRAM_VEL_ON || (s.velocity == GRAM_VEL_OFF && on);
  }
  if ((v = (unsigned)(col - g.velocity0)) < (unsigned)g.n_velocity) return body;
  if ((v = (unsigned)(col - g.program0)) < (unsigned)g.n_program) return true;
  if ((v = (unsigned)(col - g.drum0)) < (unsigned)g.n_drum) return body && s.velocity == GRAM_VEL_ON;
  return false;   // pad, unk, ids outside the codec
}

// mrow[c] = 1 where the row may not emit c next (not allowed, or banned by the static mask).  One wave.
__device__ __forceinline__ void gram_write_mask(const mrmt3_grammar& g, const GramS& s, const unsigned (&act)[4],
                                                const unsigned (&car)[4], bool has_carry,
                                                const uint8_t* __restrict__ sban, int V, uint8_t* __restrict__ mrow, int lane) {
  if ((V & 3) == 0) {       // rows of the mask are 4-byte aligned: one store per four columns
    for (int c = lane * 4; c < V; c += 256) {
      unsigned w = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool banned = !gram_allowed(g, s, act, car, has_carry, c + j) || (sban != nullptr && sban[c + j]);
        w |= (banned ? 1u : 0u) << (8 * j);
      }
      *(unsigned*)(mrow + c) = w;
    }
  } else {
    for (int c = lane; c < V; c += 64)
      mrow[c] = (!gram_allowed(g, s, act, car, has_carry, c) || (sban != nullptr && sban[c])) ? 1 : 0;
  }
}

// The 128-bit slice of a row's carry for `program` (zeros without a carry or a program).
__device__ __forceinline__ void gram_carry_slice(const uint8_t* __restrict__ carry_row, int program, unsigned (&car)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    car[j] = (carry_row != nullptr && program >= 0) ? ((const unsigned*)carry_row)[program * 4 + j] : 0u;
}

// One wave: `dst` = `src` (the parent's state) after `tok`, and the row's next mask.
__device__ __forceinline__ void gram_advance_row(const mrmt3_grammar& g, const GramRow* __restrict__ src,
                                                 GramRow* __restrict__ dst, const uint8_t* __restrict__ carry_row,
                                                 const uint8_t* __restrict__ sban, int tok, int V,
                                                 uint8_t* __restrict__ mrow, int lane) {
  const u32x4 lo = ((const u32x4*)src->active)[lane * 2], hi = ((const u32x4*)src->active)[lane * 2 + 1];
  unsigned a[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  GramS s = src->s;
  int idx;
  const int op = gram_push(g, s, tok, idx);
  if (op != GRAM_OP_NONE && (idx >> 8) == lane) {        // word idx >> 5 lives in lane (idx >> 5) >> 3
    const unsigned bit = 1u << (idx & 31);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (((idx >> 5) & 7) == e) a[e] = op == GRAM_OP_SET ? (a[e] | bit) : (a[e] & ~bit);
  }
  u32x4 o0, o1;
  o0.x = a[0]; o0.y = a[1]; o0.z = a[2]; o0.w = a[3]; o1.x = a[4]; o1.y = a[5]; o1.z = a[6]; o1.w = a[7];
  ((u32x4*)dst->active)[lane * 2] = o0;
  ((u32x4*)dst->active)[lane * 2 + 1] = o1;
  if (lane == 0) dst->s = s;
  // the slice of the program now in force: words 4 p .. 4 p + 3 sit in lane p >> 1, upper or lower half
  unsigned act[4], car[4];
  const int p = max(s.program, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned mine = (p & 1) ? a[4 + j] : a[j];
    act[j] = s.program >= 0 ? (unsigned)__shfl((int)mine, p >> 1, 64) : 0u;
  }
  gram_carry_slice(carry_row, s.program, car);
  gram_write_mask(g, s, act, car, carry_row != nullptr, sban, V, mrow, lane);
}

// Start state of every row and its first mask.  One wave per row, 8 rows per workgroup.
__global__ __launch_bounds__(512) void gram_init_kernel(const mrmt3_grammar* __restrict__ gd, mrmt3_grammar gv, GramHdr* hdr,
                                                        GramRow* __restrict__ rows0, const uint8_t* __restrict__ carry,
                                                        const uint8_t* __restrict__ sban, int rows, int V,
                                                        uint8_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (hdr != nullptr && blockIdx.x == 0 && threadIdx.x == 0) { hdr->parity = 0; hdr->carry = carry; hdr->ban = sban; }
  if (r >= rows) return;
  const mrmt3_grammar g = gd ? *gd : gv;
  const uint8_t* crow = carry ? carry + (size_t)r * MRMT3_GRAMMAR_SET_BYTES : nullptr;
  GramRow* dst = rows0 + r;
  // a row that starts in the body (no tie section) starts with what was sounding; one that starts in the tie section
  // declares its own set
  const bool seed = !g.tie_section && crow != nullptr;
  u32x4 z0 = {0u, 0u, 0u, 0u}, z1 = z0;
  if (seed) { z0 = ((const u32x4*)crow)[lane * 2]; z1 = ((const u32x4*)crow)[lane * 2 + 1]; }
  ((u32x4*)dst->active)[lane * 2] = z0;
  ((u32x4*)dst->active)[lane * 2 + 1] = z1;
  GramS s;
  s.mode = g.tie_section ? GRAM_TIE : GRAM_BODY; s.program = -1; s.velocity = GRAM_VEL_UNSET; s.cur = 0; s.acc = 0;
  if (lane == 0) dst->s = s;
  const unsigned none[4] = {0u, 0u, 0u, 0u};       // no program yet: no pitch is allowed, the slices do not matter
  gram_write_mask(g, s, none, none, crow != nullptr, sban, V, mask + (size_t)r * V, lane);
}

// The decoder's step kernel, after the tail: the tail has written step t's tokens (and, under beam search, parents) and
// advanced the step counter.
__global__ __launch_bounds__(512) void dec_grammar_step(const mrmt3_grammar* __restrict__ gd, char* __restrict__ blob,
                                                        int max_rows, const int64_t* __restrict__ tokens, int tok_ld,
                                                        const int* __restrict__ state, const int* __restrict__ bp, int rows,
                                                        int V, int pad, uint8_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 8 + (threadIdx.x >> 6);
  const int p = state[ST_T] - 1, npre = state[ST_NPRE];      // the position the tail has just closed
  if (p + 1 <= npre || r >= rows) return;                    // a prefix step emitted nothing
  const int t = p - npre;
  const int tok = (int)tokens[(size_t)r * tok_ld + t + 1];
  if (tok == pad) return;                                    // the row (beam: its group) had finished before this step
  const mrmt3_grammar g = *gd;
  const GramHdr* hdr = (const GramHdr*)blob;                 // carry and static ban of this decode (mrmt3_decoder_set_grammar)
  GramRow* buf = (GramRow*)(blob + sizeof(GramHdr));
  const int parent = bp ? bp[((size_t)t * rows + r) * 2] : r;
  const GramRow* src = buf + (size_t)(t & 1) * max_rows + parent;
  GramRow* dst = buf + (size_t)((t + 1) & 1) * max_rows + r;
  gram_advance_row(g, src, dst, hdr->carry ? hdr->carry + (size_t)r * MRMT3_GRAMMAR_SET_BYTES : nullptr, hdr->ban, tok, V,
                   mask + (size_t)r * V, lane);
}

// The same on a caller's state (mrmt3_grammar_advance); gram_flip_kernel then makes the written copy current.
__global__ __launch_bounds__(512) void gram_advance_kernel(mrmt3_grammar g, char* __restrict__ blob,
                                                           const int32_t* __restrict__ parents,
                                                           const int64_t* __restrict__ tokens, int rows, int V, int pad,
                                                           uint8_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const GramHdr* hdr = (const GramHdr*)blob;
  GramRow* buf = (GramRow*)(blob + sizeof(GramHdr));
  const int par = hdr->parity & 1;
  const int tok = (int)tokens[r];
  // a padded row keeps ITS state: carried over to the copy that becomes current, mask untouched
  const bool idle = tok == pad;
  const int parent = (parents && !idle && (unsigned)parents[r] < (unsigned)rows) ? parents[r] : r;
  const GramRow* src = buf + (size_t)par * rows + parent;
  GramRow* dst = buf + (size_t)(par ^ 1) * rows + r;
  if (idle) {
    ((u32x4*)dst->active)[lane * 2] = ((const u32x4*)src->active)[lane * 2];
    ((u32x4*)dst->active)[lane * 2 + 1] = ((const u32x4*)src->active)[lane * 2 + 1];
    if (lane == 0) dst->s = src->s;
    return;
  }
  gram_advance_row(g, src, dst, hdr->carry ? hdr->carry + (size_t)r * MRMT3_GRAMMAR_SET_BYTES : nullptr, hdr->ban, tok, V,
                   mask + (size_t)r * V, lane);
}
__global__ void gram_flip_kernel(GramHdr* hdr) { hdr->parity ^= 1; }

__global__ __launch_bounds__(512) void gram_active_kernel(const char* __restrict__ blob, int rows, uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const GramHdr* hdr = (const GramHdr*)blob;
  const GramRow* src = (const GramRow*)(blob + sizeof(GramHdr)) + (size_t)(hdr->parity & 1) * rows + r;
  u32x4* o = (u32x4*)(out + (size_t)r * MRMT3_GRAMMAR_SET_BYTES);
  o[lane * 2] = ((const u32x4*)src->active)[lane * 2];
  o[lane * 2 + 1] = ((const u32x4*)src->active)[lane * 2 + 1];
}

// The `active` set a row's emitted tokens leave behind, pushed again from the start state (mrmt3_decoder_grammar_active):
// ids[r * ld + 1 ..] up to EOS, pad or `limit` tokens (*limit_dev - npre when limit < 0: the token steps run so far).
// One wave per row; the set lives in LDS and lane 0 walks the tokens.
__global__ __launch_bounds__(64) void gram_replay_kernel(const mrmt3_grammar* __restrict__ gd, mrmt3_grammar gv,
                                                         const int64_t* __restrict__ ids,
                                                         int ld, int limit, const int* __restrict__ state,
                                                         const uint8_t* __restrict__ carry, int carry_row_stride,
                                                         uint8_t* __restrict__ out) {
  __shared__ unsigned act[GRAM_WORDS];
  const int lane = threadIdx.x, r = blockIdx.x;
  const mrmt3_grammar g = gd ? *gd : gv;
  const unsigned* crow = carry ? (const unsigned*)(carry + (size_t)r * carry_row_stride * MRMT3_GRAMMAR_SET_BYTES) : nullptr;
  for (int w = lane; w < GRAM_WORDS; w += 64) act[w] = (!g.tie_section && crow) ? crow[w] : 0u;
  __syncthreads();
  if (lane == 0) {
    GramS s;
    s.mode = g.tie_section ? GRAM_TIE : GRAM_BODY; s.program = -1; s.velocity = GRAM_VEL_UNSET; s.cur = 0; s.acc = 0;
    const int n = limit >= 0 ? limit : state[ST_T] - state[ST_NPRE];
    for (int t = 0; t < n && t + 1 < ld; ++t) {
      const int tok = (int)ids[(size_t)r * ld + t + 1];
      if (tok == g.eos || tok == g.pad) break;
      int idx;
      const int op = gram_push(g, s, tok, idx);
      if (op == GRAM_OP_SET) act[idx >> 5] |= 1u << (idx & 31);
      else if (op == GRAM_OP_CLEAR) act[idx >> 5] &= ~(1u << (idx & 31));
    }
  }
  __syncthreads();
  unsigned* o = (unsigned*)(out + (size_t)r * MRMT3_GRAMMAR_SET_BYTES);
  for (int w = lane; w < GRAM_WORDS; w += 64) o[w] = act[w];
}

__global__ void gram_desc_set_kernel(mrmt3_grammar* rec, mrmt3_grammar v) { *rec = v; }

// position 0 becomes the first memory row instead of the start token
__global__ void dec_prefix_kernel(int B, int n_prefix, const float* prefix, const float* pos, float* x, int* state) {
  const int tid = threadIdx.x;
  if (tid == 0) state[ST_NPRE] = n_prefix;
  for (int b = 0; b < B; ++b) {
    const float* er = prefix + (size_t)b * n_prefix * DMODEL;
    x[b * DMODEL + tid] = er[tid] + pos[tid];
    x[b * DMODEL + 256 + tid] = er[256 + tid] + pos[256 + tid];
  }
}

__global__ void dec_begin_kernel(int B, int64_t* tokens, int tok_ld, const float* embed, const float* pos, float* x,
                                 int* state, int start_id) {
  const int tid = threadIdx.x;
  for (int i = tid; i <= ST_CNT; i += (int)blockDim.x) state[i] = (i == ST_FIN) ? -1 : 0;
  for (int b = 0; b < B; ++b) {
    if (tid == 0) tokens[(size_t)b * tok_ld] = start_id;
    x[b * DMODEL + tid] = embed[(size_t)start_id * DMODEL + tid] + pos[tid];
    x[b * DMODEL + 256 + tid] = embed[(size_t)start_id * DMODEL + 256 + tid] + pos[256 + tid];
  }
}

// ------------------------------------------------------------------------------------------------
struct mrmt3_decoder {
  int L, d, H, dff, V, maxB, maxLen, maxEnc, wdt, inner;
  float eps;
  void *kc, *vc;  // [L][maxB][maxLen][inner]
  float *x, *q, *o, *g, *logits;
  float* blp;     // beam search: [2][maxLen][maxB] f32 log-probabilities beside the backpointers (dec_beam_select)
  SampleCfg* samp;   // sampling parameters and seed, read by dec_sample at every step (mrmt3_decoder_set_sampling)
  int* state;
  // per-batch
  mrmt3_decoder_weights w;
  const void *ln_self[64], *w_qkv[64], *w_o_self[64], *ln_cross[64], *w_q_cross[64], *w_o_cross[64], *ln_ff[64],
      *w_wi[64], *w_wo[64];
  const void* cross_kv;
  const float* prefix;   // [B][n_prefix][d] f32 memory rows fed before the start token (or null)
  int B, encLen, eos, pad, start;
  int64_t* tokens;
  // what the step's tail bakes into the graph: k = 0 greedy (ban = null: the plain argmax), k > 0 beam search
  struct Tail {
    int k, groups;
    float length_penalty;
    const uint8_t* ban;
    int ban_stride;   // 0: `ban` is one static [V] mask; V: the event grammar's mask per row (`gram`)
    int gram;         // 1: dec_grammar_step follows the tail (mrmt3_decoder_set_grammar)
    float* logp;      // greedy: per-token log-probabilities [B][logp_ld] (null = off: the plain / banned argmax)
    int logp_ld;
    int sample;       // 1: dec_sample draws the token (its parameters live in `samp`, not here: they may change per call)
    float* bscore;
    int* bp;
    int* hyp;
  } tail;
  Tail cap_tail;    // tail of the captured graph
  int n_prefix;     // set by mrmt3_decoder_set_prefix since the last begin
  hipGraph_t graph;
  hipGraphExec_t exec;
  int captured;     // 1 = exec valid for the current (B, encLen, pointers)
  int graph_failed;  // 1 = capture failed once; run with plain launches
  int captures;      // step graphs instantiated so far (mrmt3_decoder_capture_count)
  // event grammar (mrmt3_decoder_set_grammar), allocated on first use and kept: the step graph bakes the addresses in
  char* gblob;             // GramHdr + 2 x maxB GramRow
  uint8_t* gmask;          // [maxB][V]
  mrmt3_grammar* gdesc;    // the descriptor, read by the step at every replay
  const uint8_t* gcarry;   // this decode's carry (also in the blob's header)
  const uint8_t* gsban;    // the static mask that was in force when the grammar went on
  const int64_t* beam_out; // what the last mrmt3_decoder_beam_finalize wrote, for mrmt3_decoder_grammar_active
  int beam_out_ld, beam_out_len;
};

extern "C" int mrmt3_decoder_create(mrmt3_decoder** out, int n_layers, int d_model, int n_heads, int d_ff, int vocab,
                                    int max_batch, int max_len, int max_enc_len, int w_dtype, float eps) {
  MR_CHECK_ARG(out, "decoder_create: null out");
  *out = nullptr;
  MR_CHECK_ARG(d_model == DMODEL, "decoder_create: kernels are specialised for d_model = 512");
  MR_CHECK_ARG(n_layers > 0 && n_layers <= 64 && max_batch > 0 && max_batch <= DEC_MAXB, "decoder_create: need 1..64 layers, batch <= 256");
  MR_CHECK_ARG(d_ff % 8 == 0 && d_ff <= 1024 && n_heads * 64 <= 512 && vocab > 0 && max_len > 0 && max_enc_len > 0, "decoder_create: need d_ff <= 1024, heads*64 <= 512");
  MR_CHECK_ARG(w_dtype == MRMT3_F32 || w_dtype == MRMT3_BF16, "decoder_create: bad dtype");
  mrmt3_decoder* D = new mrmt3_decoder();
  memset(D, 0, sizeof(*D));
  D->L = n_layers; D->d = d_model; D->H = n_heads; D->dff = d_ff; D->V = vocab; D->maxB = max_batch;
  D->maxLen = max_len; D->maxEnc = max_enc_len; D->wdt = w_dtype; D->inner = n_heads * 64; D->eps = eps;
  const size_t esz = w_dtype == MRMT3_BF16 ? 2 : 4;
  const size_t cache = (size_t)n_layers * max_batch * max_len * D->inner * esz;
  hipError_t e = hipMalloc(&D->kc, cache);
  if (e == hipSuccess) e = hipMalloc(&D->vc, cache);
  if (e == hipSuccess) e = hipMalloc((void**)&D->x, sizeof(float) * max_batch * DMODEL);
  if (e == hipSuccess) e = hipMalloc((void**)&D->q, sizeof(float) * max_batch * D->inner);
  if (e == hipSuccess) e = hipMalloc((void**)&D->o, sizeof(float) * max_batch * D->inner);
  if (e == hipSuccess) e = hipMalloc((void**)&D->g, sizeof(float) * max_batch * d_ff);
  if (e == hipSuccess) e = hipMalloc((void**)&D->logits, sizeof(float) * max_batch * vocab);
  if (e == hipSuccess) e = hipMalloc((void**)&D->state, sizeof(int) * (ST_CNT + 1));
  if (e == hipSuccess) e = hipMalloc((void**)&D->blp, sizeof(float) * 2 * max_len * max_batch);
  if (e == hipSuccess) e = hipMalloc((void**)&D->samp, sizeof(SampleCfg));
  if (e != hipSuccess) {
    mrmt3_set_error("decoder_create: hipMalloc failed: %s", hipGetErrorString(e));
    mrmt3_decoder_destroy(D);
    return MRMT3_ERR_HIP;
  }
  *out = D;
  return MRMT3_OK;
}

extern "C" void mrmt3_decoder_destroy(mrmt3_decoder* D) {
  if (!D) return;
  if (D->exec) (void)hipGraphExecDestroy(D->exec);
  if (D->graph) (void)hipGraphDestroy(D->graph);
  void* bufs[] = {D->kc, D->vc, D->x, D->q, D->o, D->g, D->logits, D->state, D->blp, D->samp, D->gblob, D->gmask, D->gdesc};
  for (void* b : bufs) if (b) (void)hipFree(b);
  delete D;
}

extern "C" int mrmt3_decoder_begin(mrmt3_decoder* D, const mrmt3_decoder_weights* w, const void* cross_kv, int batch,
                                   int enc_len, int64_t* tokens_out, int start_id, int eos_id, int pad_id,
                                   void* stream) {
  MR_CHECK_ARG(D && w && cross_kv && tokens_out, "decoder_begin: null pointer");
  MR_CHECK_ARG(batch > 0 && batch <= D->maxB && enc_len > 0 && enc_len <= D->maxEnc, "decoder_begin: batch/enc_len out of range");
  bool same = D->captured && D->B == batch && D->encLen == enc_len && D->cross_kv == cross_kv &&
              D->tokens == tokens_out && D->eos == eos_id && D->pad == pad_id && D->w.embed == w->embed &&
              D->w.lm_head == w->lm_head && D->w.pos == w->pos && D->w.final_ln == w->final_ln;
  for (int l = 0; l < D->L && same; ++l)
    same = D->w_qkv[l] == w->w_qkv[l] && D->w_wi[l] == w->w_wi[l] && D->w_wo[l] == w->w_wo[l] &&
           D->w_o_self[l] == w->w_o_self[l] && D->w_q_cross[l] == w->w_q_cross[l] && D->w_o_cross[l] == w->w_o_cross[l];
  D->w = *w;
  for (int l = 0; l < D->L; ++l) {
    D->ln_self[l] = w->ln_self[l]; D->w_qkv[l] = w->w_qkv[l]; D->w_o_self[l] = w->w_o_self[l];
    D->ln_cross[l] = w->ln_cross[l]; D->w_q_cross[l] = w->w_q_cross[l]; D->w_o_cross[l] = w->w_o_cross[l];
    D->ln_ff[l] = w->ln_ff[l]; D->w_wi[l] = w->w_wi[l]; D->w_wo[l] = w->w_wo[l];
  }
  D->cross_kv = cross_kv; D->B = batch; D->encLen = enc_len; D->tokens = tokens_out; D->eos = eos_id; D->pad = pad_id;
  D->start = start_id;
  if (!same) D->captured = 0;
  memset(&D->tail, 0, sizeof(D->tail));
  D->n_prefix = 0;
  D->gcarry = nullptr; D->beam_out = nullptr;
  hipLaunchKernelGGL(dec_begin_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, batch, tokens_out, D->maxLen + 1,
                     (const float*)w->embed, w->pos, D->x, D->state, start_id);
  MR_CHECK_LAUNCH("decoder_begin");
  return MRMT3_OK;
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

// ---- event grammar entry points --------------------------------------------------------------------------------
static int grammar_check(const char* who, const mrmt3_grammar* g, int V) {
  MR_CHECK_ARG(g != nullptr, "%s: null grammar", who);
  const int r[5][2] = {{g->shift0, g->n_shift}, {g->pitch0, g->n_pitch}, {g->velocity0, g->n_velocity},
                       {g->program0, g->n_program}, {g->drum0, g->n_drum}};
  for (int i = 0; i < 5; ++i)
    MR_CHECK_ARG(r[i][0] >= 0 && r[i][1] >= 1 && (long)r[i][0] + r[i][1] <= V, "%s: id range %d (%d + %d) outside the vocabulary %d",
                 who, i, r[i][0], r[i][1], V);
  MR_CHECK_ARG(g->n_pitch <= 128 && g->n_program <= 128, "%s: the state holds 128 x 128 (program, pitch) pairs", who);
  MR_CHECK_ARG(g->n_velocity >= 2, "%s: need an off and an on velocity", who);
  MR_CHECK_ARG(g->tie >= 0 && g->tie < V && g->eos >= 0 && g->eos < V && g->pad >= 0 && g->pad < V && g->eos != g->pad,
               "%s: tie / eos / pad ids outside the vocabulary %d", who, V);
  MR_CHECK_ARG(g->max_shift_steps >= 0, "%s: max_shift_steps < 0", who);
  return MRMT3_OK;
}

extern "C" size_t mrmt3_grammar_state_bytes(int rows) {
  return rows > 0 ? sizeof(GramHdr) + 2 * (size_t)rows * sizeof(GramRow) : 0;
}

extern "C" int mrmt3_grammar_init(const mrmt3_grammar* g, void* state, const uint8_t* carry, const uint8_t* banned_mask,
                                  int rows, int V, uint8_t* mask_out, void* stream) {
  MR_CHECK_ARG(state && mask_out && rows > 0 && V > 0, "grammar_init: bad args");
  MR_CHECK_ARG(((uintptr_t)state & 15) == 0, "grammar_init: state must be 16-byte aligned");
  int rc = grammar_check("grammar_init", g, V);
  if (rc != MRMT3_OK) return rc;
  hipLaunchKernelGGL(gram_init_kernel, dim3((unsigned)ceil_div(rows, 8)), dim3(512), 0, (hipStream_t)stream,
                     (const mrmt3_grammar*)nullptr, *g, (GramHdr*)state, (GramRow*)((char*)state + sizeof(GramHdr)), carry,
                     banned_mask, rows, V, mask_out);
  MR_CHECK_LAUNCH("grammar_init");
  return MRMT3_OK;
}

extern "C" int mrmt3_grammar_advance(const mrmt3_grammar* g, void* state, const int32_t* parents, const int64_t* tokens,
                                     int rows, int V, uint8_t* mask_out, void* stream) {
  MR_CHECK_ARG(state && tokens && mask_out && rows > 0 && V > 0, "grammar_advance: bad args");
  int rc = grammar_check("grammar_advance", g, V);
  if (rc != MRMT3_OK) return rc;
  hipLaunchKernelGGL(gram_advance_kernel, dim3((unsigned)ceil_div(rows, 8)), dim3(512), 0, (hipStream_t)stream, *g,
                     (char*)state, parents, tokens, rows, V, g->pad, mask_out);
  hipLaunchKernelGGL(gram_flip_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (GramHdr*)state);
  MR_CHECK_LAUNCH("grammar_advance");
  return MRMT3_OK;
}

extern "C" int mrmt3_grammar_active(const void* state, int rows, uint8_t* out, void* stream) {
  MR_CHECK_ARG(state && out && rows > 0, "grammar_active: bad args");
  hipLaunchKernelGGL(gram_active_kernel, dim3((unsigned)ceil_div(rows, 8)), dim3(512), 0, (hipStream_t)stream,
                     (const char*)state, rows, out);
  MR_CHECK_LAUNCH("grammar_active");
  return MRMT3_OK;
}

extern "C" int mrmt3_grammar_replay(const mrmt3_grammar* g, const int64_t* ids, int ld, int rows, int n_tokens, int V,
                                    const uint8_t* carry, uint8_t* out, void* stream) {
  MR_CHECK_ARG(ids && out && rows > 0 && ld >= 1 && n_tokens >= 0, "grammar_replay: bad args");
  int rc = grammar_check("grammar_replay", g, V);
  if (rc != MRMT3_OK) return rc;
  hipLaunchKernelGGL(gram_replay_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, (const mrmt3_grammar*)nullptr,
                     *g, ids, ld, n_tokens, (const int*)nullptr, carry, 1, out);
  MR_CHECK_LAUNCH("grammar_replay");
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_set_grammar(mrmt3_decoder* D, const mrmt3_grammar* g, const uint8_t* carry, void* stream) {
  MR_CHECK_ARG(D && D->tokens, "decoder_set_grammar: call decoder_begin first");
  mrmt3_decoder::Tail& T = D->tail;
  if (!g) {
    if (T.gram) { T.ban = D->gsban; T.gram = 0; T.ban_stride = 0; }
    return MRMT3_OK;
  }
  MR_CHECK_ARG(!T.gram, "decoder_set_grammar: already set for this decode");
  int rc = grammar_check("decoder_set_grammar", g, D->V);
  if (rc != MRMT3_OK) return rc;
  MR_CHECK_ARG(g->eos == D->eos && g->pad == D->pad, "decoder_set_grammar: eos / pad differ from decoder_begin's");
  if (!D->gblob) {
    hipError_t e = hipMalloc((void**)&D->gblob, mrmt3_grammar_state_bytes(D->maxB));
    if (e == hipSuccess) e = hipMalloc((void**)&D->gmask, (size_t)D->maxB * D->V);
    if (e == hipSuccess) e = hipMalloc((void**)&D->gdesc, sizeof(mrmt3_grammar));
    if (e != hipSuccess) {
      mrmt3_set_error("decoder_set_grammar: hipMalloc failed: %s", hipGetErrorString(e));
      return MRMT3_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(gram_desc_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, D->gdesc, *g);
  // the static mask in force (greedy: mrmt3_decoder_set_ban, beam: mrmt3_decoder_begin_beam) goes into the row masks
  hipLaunchKernelGGL(gram_init_kernel, dim3((unsigned)ceil_div(D->B, 8)), dim3(512), 0, (hipStream_t)stream,
                     (const mrmt3_grammar*)nullptr, *g, (GramHdr*)D->gblob, (GramRow*)(D->gblob + sizeof(GramHdr)), carry,
                     T.ban, D->B, D->V, D->gmask);
  MR_CHECK_LAUNCH("decoder_set_grammar");
  D->gcarry = carry; D->gsban = T.ban;
  T.ban = D->gmask; T.ban_stride = D->V; T.gram = 1;
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_grammar_active(mrmt3_decoder* D, uint8_t* out, void* stream) {
  MR_CHECK_ARG(D && out && D->tokens && D->tail.gram, "decoder_grammar_active: no constrained decode on the handle");
  const mrmt3_decoder::Tail& T = D->tail;
  if (T.k > 0) {
    MR_CHECK_ARG(D->beam_out, "decoder_grammar_active: call decoder_beam_finalize first");
    hipLaunchKernelGGL(gram_replay_kernel, dim3((unsigned)T.groups), dim3(64), 0, (hipStream_t)stream,
                       (const mrmt3_grammar*)D->gdesc, mrmt3_grammar{}, D->beam_out, D->beam_out_ld, D->beam_out_len,
                       (const int*)D->state,
                       D->gcarry, T.k, out);
  } else {
    hipLaunchKernelGGL(gram_replay_kernel, dim3((unsigned)D->B), dim3(64), 0, (hipStream_t)stream,
                       (const mrmt3_grammar*)D->gdesc, mrmt3_grammar{}, (const int64_t*)D->tokens, D->maxLen + 1, -1,
                       (const int*)D->state,
                       D->gcarry, 1, out);
  }
  MR_CHECK_LAUNCH("decoder_grammar_active");
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

extern "C" int mrmt3_decoder_set_prefix(mrmt3_decoder* D, const float* prefix, int n_prefix, void* stream) {
  MR_CHECK_ARG(D && D->tokens, "decoder_set_prefix: call decoder_begin first");
  MR_CHECK_ARG(prefix && n_prefix > 0 && n_prefix < D->maxLen, "decoder_set_prefix: need 0 < n_prefix < max_len rows");
  MR_CHECK_ARG(D->tail.k == 0, "decoder_set_prefix: not available in beam mode");
  D->n_prefix = n_prefix;
  if (D->prefix != prefix) { D->prefix = prefix; D->captured = 0; }   // pointer is baked into the graph
  hipLaunchKernelGGL(dec_prefix_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, D->B, n_prefix, prefix, D->w.pos,
                     D->x, D->state);
  MR_CHECK_LAUNCH("decoder_set_prefix");
  return MRMT3_OK;
}

template <typename TW>
static int launch_step(mrmt3_decoder* D, hipStream_t s);

// the step's last kernel(s): greedy argmax (banned or not), the sampled tail, or the beam select + KV-cache reorder
static void launch_tail(mrmt3_decoder* D, hipStream_t s) {
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
  if (D->tail.gram)
    hipLaunchKernelGGL(dec_grammar_step, dim3((unsigned)ceil_div(B, 8)), dim3(512), 0, s, (const mrmt3_grammar*)D->gdesc,
                       D->gblob, D->maxB, (const int64_t*)D->tokens, D->maxLen + 1, (const int*)D->state,
                       D->tail.k > 0 ? (const int*)D->tail.bp : (const int*)nullptr, B, V, D->pad, D->gmask);
}

// batch > 8, bf16 weights: projections on the matrix cores, 16 sequences per wave
static int launch_step_mfma(mrmt3_decoder* D, hipStream_t s) {
  typedef bf16_t TW;
  const int B = D->B, inner = D->inner, dff = D->dff, V = D->V;
  const size_t cache_b = (size_t)D->maxLen * inner;
  const size_t cache_l = (size_t)D->maxB * cache_b;
  const size_t attn_extra = (size_t)(64 + 8 + 32 * 64) * sizeof(float);
  const size_t attn_shm_self = (size_t)((D->maxLen + 3) & ~3) * sizeof(float) + attn_extra;
  const size_t attn_shm_cross = (size_t)((D->encLen + 3) & ~3) * sizeof(float) + attn_extra;
  const TW* ckv = (const TW*)D->cross_kv;
  const dim3 blk(256);
  auto rows = [&](int n) { return dim3((unsigned)ceil_div(n, 16), (unsigned)ceil_div(B, 16)); };
  for (int l = 0; l < D->L; ++l) {
    TW* kc = (TW*)D->kc + l * cache_l;
    TW* vc = (TW*)D->vc + l * cache_l;
    hipLaunchKernelGGL((dec_norm_gemm16<1>), rows(3 * inner), blk, 0, s, D->x, (const float*)D->ln_self[l],
                       (const TW*)D->w_qkv[l], 3 * inner, D->eps, D->q, kc, vc, inner, cache_b, D->state, B);
    hipLaunchKernelGGL((dec_attn<TW>), dim3(D->H, B), dim3(256), attn_shm_self, s, D->q, (const TW*)kc, (const TW*)vc,
                       inner, cache_b, 0, D->state, D->o, inner);
    hipLaunchKernelGGL((dec_gemm16_res<3>), rows(DMODEL), blk, 0, s, D->o, (const TW*)D->w_o_self[l], D->x, DMODEL, B);
    hipLaunchKernelGGL((dec_norm_gemm16<0>), rows(inner), blk, 0, s, D->x, (const float*)D->ln_cross[l],
                       (const TW*)D->w_q_cross[l], inner, D->eps, D->q, (TW*)nullptr, (TW*)nullptr, inner, (size_t)0,
                       D->state, B);
    const TW* ck = ckv + (size_t)l * B * D->encLen * 2 * inner;
    hipLaunchKernelGGL((dec_attn<TW>), dim3(D->H, B), dim3(256), attn_shm_cross, s, D->q, ck, ck + inner, 2 * inner,
                       (size_t)D->encLen * 2 * inner, D->encLen, D->state, D->o, inner);
    hipLaunchKernelGGL((dec_gemm16_res<3>), rows(DMODEL), blk, 0, s, D->o, (const TW*)D->w_o_cross[l], D->x, DMODEL, B);
    hipLaunchKernelGGL((dec_norm_gemm16<2>), rows(dff), blk, 0, s, D->x, (const float*)D->ln_ff[l],
                       (const TW*)D->w_wi[l], dff, D->eps, D->g, (TW*)nullptr, (TW*)nullptr, inner, (size_t)0, D->state, B);
    hipLaunchKernelGGL((dec_gemm16_res<8>), rows(DMODEL), blk, 0, s, D->g, (const TW*)D->w_wo[l], D->x, DMODEL, B);
  }
  hipLaunchKernelGGL((dec_norm_gemm16<0>), rows(V), blk, 0, s, D->x, D->w.final_ln, (const TW*)D->w.lm_head, V, D->eps,
                     D->logits, (TW*)nullptr, (TW*)nullptr, inner, (size_t)0, D->state, B);
  launch_tail(D, s);
  MR_CHECK_LAUNCH("decoder step (mfma)");
  return MRMT3_OK;
}

template <typename TW>
static int launch_step(mrmt3_decoder* D, hipStream_t s) {
  const int B = D->B, inner = D->inner, dff = D->dff, V = D->V;
  const size_t cache_b = (size_t)D->maxLen * inner;             // elements per batch row of a layer's cache
  const size_t cache_l = (size_t)D->maxB * cache_b;             // elements per layer
  const size_t attn_extra = (size_t)(64 + 8 + 32 * 64) * sizeof(float);
  const size_t attn_shm_self = (size_t)((D->maxLen + 3) & ~3) * sizeof(float) + attn_extra;
  const size_t attn_shm_cross = (size_t)((D->encLen + 3) & ~3) * sizeof(float) + attn_extra;
  const TW* ckv = (const TW*)D->cross_kv;
  const dim3 blk(64 * DEC_WPG);
  auto rows = [&](int n) { return dim3((unsigned)ceil_div(n, DEC_WPG), (unsigned)B); };
  for (int l = 0; l < D->L; ++l) {
    TW* kc = (TW*)D->kc + l * cache_l;
    TW* vc = (TW*)D->vc + l * cache_l;
    hipLaunchKernelGGL((dec_norm_gemv<TW, 1>), rows(3 * inner), blk, 0, s, D->x, (const float*)D->ln_self[l],
                       (const TW*)D->w_qkv[l], 3 * inner, D->eps, D->q, kc, vc, inner, cache_b, D->state);
    hipLaunchKernelGGL((dec_attn<TW>), dim3(D->H, B), dim3(256), attn_shm_self, s, D->q, (const TW*)kc, (const TW*)vc,
                       inner, cache_b, 0, D->state, D->o, inner);
    hipLaunchKernelGGL((dec_gemv_res<TW, 1>), rows(DMODEL), blk, 0, s, D->o, (const TW*)D->w_o_self[l], D->x, DMODEL,
                       inner);
    hipLaunchKernelGGL((dec_norm_gemv<TW, 0>), rows(inner), blk, 0, s, D->x, (const float*)D->ln_cross[l],
                       (const TW*)D->w_q_cross[l], inner, D->eps, D->q, (TW*)nullptr, (TW*)nullptr, inner, (size_t)0,
                       D->state);
    const TW* ck = ckv + (size_t)l * B * D->encLen * 2 * inner;
    hipLaunchKernelGGL((dec_attn<TW>), dim3(D->H, B), dim3(256), attn_shm_cross, s, D->q, ck, ck + inner, 2 * inner,
                       (size_t)D->encLen * 2 * inner, D->encLen, D->state, D->o, inner);
    hipLaunchKernelGGL((dec_gemv_res<TW, 1>), rows(DMODEL), blk, 0, s, D->o, (const TW*)D->w_o_cross[l], D->x, DMODEL,
                       inner);
    hipLaunchKernelGGL((dec_norm_gemv<TW, 2>), rows(dff), blk, 0, s, D->x, (const float*)D->ln_ff[l],
                       (const TW*)D->w_wi[l], dff, D->eps, D->g, (TW*)nullptr, (TW*)nullptr, inner, (size_t)0, D->state);
    hipLaunchKernelGGL((dec_gemv_res<TW, 2>), rows(DMODEL), blk, 0, s, D->g, (const TW*)D->w_wo[l], D->x, DMODEL, dff);
  }
  hipLaunchKernelGGL((dec_norm_gemv<TW, 0>), rows(V), blk, 0, s, D->x, D->w.final_ln, (const TW*)D->w.lm_head, V, D->eps,
                     D->logits, (TW*)nullptr, (TW*)nullptr, inner, (size_t)0, D->state);
  launch_tail(D, s);
  MR_CHECK_LAUNCH("decoder step");
  return MRMT3_OK;
}

static int step(mrmt3_decoder* D, hipStream_t s) {
  if (D->wdt == MRMT3_BF16 && D->B > DEC_MFMA_ABOVE && D->inner == 384 && D->dff == 1024 && D->d == DMODEL)
    return launch_step_mfma(D, s);
  return D->wdt == MRMT3_BF16 ? launch_step<bf16_t>(D, s) : launch_step<float>(D, s);
}

extern "C" int mrmt3_decoder_run(mrmt3_decoder* D, int n_steps, void* stream) {
  MR_CHECK_ARG(D && D->tokens && n_steps >= 0, "decoder_run: call decoder_begin first");
  hipStream_t s = (hipStream_t)stream;
  const mrmt3_decoder::Tail &a = D->tail, &c = D->cap_tail;
  if (a.k != c.k || a.groups != c.groups || a.length_penalty != c.length_penalty || a.ban != c.ban ||
      a.ban_stride != c.ban_stride || a.gram != c.gram ||
      a.logp != c.logp || a.logp_ld != c.logp_ld || a.sample != c.sample || a.bscore != c.bscore || a.bp != c.bp || a.hyp != c.hyp)
    D->captured = 0;             // greedy <-> beam, ban <-> no ban, grammar, log-probabilities or sampling on <-> off: the tail is baked into the graph
  if (!D->captured && !D->graph_failed) {
    D->cap_tail = D->tail;
    if (D->exec) { (void)hipGraphExecDestroy(D->exec); D->exec = nullptr; }
    if (D->graph) { (void)hipGraphDestroy(D->graph); D->graph = nullptr; }
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
      int rc = step(D, s);
      hipError_t e2 = hipStreamEndCapture(s, &D->graph);
      if (rc == MRMT3_OK && e2 == hipSuccess && D->graph) e = hipGraphInstantiate(&D->exec, D->graph, nullptr, nullptr, 0);
      else e = hipErrorUnknown;
    }
    if (e == hipSuccess && D->exec) { D->captured = 1; ++D->captures; }
    else { D->graph_failed = 1; (void)hipGetLastError(); }
  }
  for (int i = 0; i < n_steps; ++i) {
    if (D->captured) {
      MR_CHECK_HIP(hipGraphLaunch(D->exec, s));
    } else {
      int rc = step(D, s);
      if (rc != MRMT3_OK) return rc;
    }
  }
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_graph_captured(const mrmt3_decoder* D) { return D ? D->captured : 0; }
extern "C" int mrmt3_decoder_capture_count(const mrmt3_decoder* D) { return D ? D->captures : 0; }

extern "C" int mrmt3_decoder_logits(mrmt3_decoder* D, float* dst, int rows, void* stream) {
  MR_CHECK_ARG(D && dst, "decoder_logits: null pointer");
  MR_CHECK_ARG(D->tokens, "decoder_logits: call decoder_begin first");
  MR_CHECK_ARG(rows > 0 && rows <= D->B, "decoder_logits: need 0 < rows <= batch (%d), got %d", D->B, rows);
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  MR_CHECK_HIP(hipStreamIsCapturing((hipStream_t)stream, &st));
  MR_CHECK_ARG(st == hipStreamCaptureStatusNone, "decoder_logits: not allowed inside a stream capture");
  MR_CHECK_HIP(hipMemcpyAsync(dst, D->logits, sizeof(float) * (size_t)rows * D->V, hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
  return MRMT3_OK;
}

extern "C" int mrmt3_decoder_poll(mrmt3_decoder* D, int32_t* state_out_pinned, void* stream) {
  MR_CHECK_ARG(D && state_out_pinned, "decoder_poll: null pointer");
  MR_CHECK_HIP(hipMemcpyAsync(state_out_pinned, D->state, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  return MRMT3_OK;
}
