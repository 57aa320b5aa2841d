// The optimizer tail: AdamW (flat and over a table of trainable ranges, with EMA weights), the step counter, the host-side
// range-table planner, and the global gradient norm with its clip coefficient and non-finite guard.
#include "common.h"
#include "opt_ranges.h"
#include "rowmath.h"

// no implicit FMA formation in this file: the AdamW update (adamw_update4: lerp, second moment, denominator, step), the
// EMA lerp and the f64 sums of squares of the gradient norm have their bits pinned under this setting
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// The optimizer tail: AdamW over the flat parameter buffer (torch.optim.AdamW single-tensor semantics), optionally under
// the clip coefficient / skip flag of the global gradient norm (Lightning's gradient_clip_val / gradient_clip_algorithm;
// torch.nn.utils.clip_grad_norm_) and optionally over a table of trainable ranges (frozen weights, per-range weight decay
// and learning-rate factor, EMA weights in the same pass).  Table layout and planner: opt_ranges.h
// ------------------------------------------------------------------------------------------------
// largest r in [lo, nr) with tab[r].start <= i   (i < tab[nr].start, tab[lo].start <= i)
__device__ __forceinline__ int opt_locate(const MrOptRec* __restrict__ tab, int lo, int nr, long long i) {
  int hi = nr;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid].start <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// The AdamW update of one 16-byte group, the only copy: gr = g * gscale (CLIP: * coef, coef = stat[1] read from the
// device — a captured graph freezes by-value arguments — then clamped to +-clip_value when that is positive).
template <bool CLIP>
__device__ __forceinline__ void adamw_update4(float pv[4], const float gv[4], float mv[4], float vv[4], float gscale,
                                              float coef, float clip_value, float decay, float b1, float b2,
                                              float bc2_sqrt, float eps, float step_size) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float gr;
    if (CLIP) {
      gr = gv[e] * gscale * coef;
      if (clip_value > 0.f) gr = gr > clip_value ? clip_value : (gr < -clip_value ? -clip_value : gr);   // NaN stays NaN
    } else {
      gr = gv[e] * gscale;
    }
    pv[e] *= decay;
    mv[e] = mv[e] + (gr - mv[e]) * (1.f - b1);             // exp_avg.lerp_(grad, 1-beta1)
    vv[e] = vv[e] * b2 + (1.f - b2) * gr * gr;             // mul_(beta2).addcmul_(g, g, 1-beta2)
    const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
    pv[e] -= step_size * (mv[e] / denom);
  }
}

// The flat form: one grid-stride loop over all n4 groups with one weight decay.  CLIP: stat[2] != 0 skips the step, every
// thread leaves before its first store.
template <bool CLIP>
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, size_t n4, const float* __restrict__ lr_dev,
                             const int32_t* __restrict__ step_dev, float b1, float b2, float eps, float wd, float gscale,
                             const float* __restrict__ stat, float clip_value, bf16_t* __restrict__ shadow) {
  float coef = 1.f;
  if (CLIP) {
    if (stat[2] != 0.f) return;
    coef = stat[1];
  }
  const float lr = lr_dev[0];
  const int step = step_dev[0] + 1;
  const double bc1 = 1.0 - pow((double)b1, (double)step);
  const double bc2 = 1.0 - pow((double)b2, (double)step);
  const float step_size = (float)((double)lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  const float decay = 1.f - lr * wd;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float pv[4], gv[4], mv[4], vv[4];
    load4<float>(p + i * 4, pv);
    load4<float>(g + i * 4, gv);
    load4<float>(m + i * 4, mv);
    load4<float>(v + i * 4, vv);
    adamw_update4<CLIP>(pv, gv, mv, vv, gscale, coef, clip_value, decay, b1, b2, bc2_sqrt, eps, step_size);
    store4<float>(p + i * 4, pv);
    store4<float>(m + i * 4, mv);
    store4<float>(v + i * 4, vv);
    if (shadow) store4<bf16_t>(shadow + i * 4, pv);
  }
}

// The range form.  A workgroup owns OG_CHUNK consecutive 16-byte groups of the virtual (trainable-only) array: one binary
// search for the range of its first group (uniform over the workgroup), then every lane walks forward from there.
// Elements outside the ranges are never addressed.  Inside a range: the flat form's update with wd and lr * lr_scale of
// the range, then ema += (1 - ema_decay) * (p_new - ema).
#define OG_PER_LANE 4
#define OG_CHUNK (256 * OG_PER_LANE)
template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           float* __restrict__ ema, const MrOptRec* __restrict__ tab, int nr,
                                                           const float* __restrict__ lr_dev,
                                                           const int32_t* __restrict__ step_dev, float b1, float b2, float eps,
                                                           float gscale, float ema_om, const float* __restrict__ stat,
                                                           float clip_value, bf16_t* __restrict__ shadow) {
  float coef = 1.f;
  if (CLIP) {
    if (stat[2] != 0.f) return;
    coef = stat[1];
  }
  const long long total = tab[nr].start;
  const long long base = (long long)blockIdx.x * OG_CHUNK;
  if (base >= total) return;
  const float lr0 = lr_dev[0];
  const int step = step_dev[0] + 1;
  const double bc1 = 1.0 - pow((double)b1, (double)step);
  const double bc2 = 1.0 - pow((double)b2, (double)step);
  const float bc2_sqrt = (float)sqrt(bc2);
  int r = opt_locate(tab, 0, nr, base);
  float step_size = 0.f, decay = 1.f;
  long long r_start = 0, r_next = 0, r_begin4 = 0;           // r_next = 0: the first group always loads its range
#pragma unroll 1
  for (int k = 0; k < OG_PER_LANE; ++k) {
    const long long i = base + (long long)k * 256 + threadIdx.x;
    if (i >= total) break;
    if (i >= r_next) {
      r = opt_locate(tab, r, nr, i);
      r_start = tab[r].start;
      r_next = tab[r + 1].start;
      r_begin4 = tab[r].begin4;
      const float lr = lr0 * tab[r].lr_scale;
      step_size = (float)((double)lr / bc1);
      decay = 1.f - lr * tab[r].wd;
    }
    const size_t o = (size_t)(r_begin4 + (i - r_start)) * 4;
    float pv[4], gv[4], mv[4], vv[4];
    load4<float>(p + o, pv);
    load4<float>(g + o, gv);
    load4<float>(m + o, mv);
    load4<float>(v + o, vv);
    adamw_update4<CLIP>(pv, gv, mv, vv, gscale, coef, clip_value, decay, b1, b2, bc2_sqrt, eps, step_size);
    store4<float>(p + o, pv);
    store4<float>(m + o, mv);
    store4<float>(v + o, vv);
    if (shadow) store4<bf16_t>(shadow + o, pv);
    if (EMA) {
      float ev[4];
      load4<float>(ema + o, ev);
#pragma unroll
      for (int e = 0; e < 4; ++e) ev[e] = ev[e] + ema_om * (pv[e] - ev[e]);
      store4<float>(ema + o, ev);
    }
  }
}

__global__ void counter_add_kernel(int32_t* ctr, int32_t delta) { ctr[0] += delta; }

extern "C" int mrmt3_counter_add(int32_t* ctr, int32_t delta, void* stream) {
  MR_CHECK_ARG(ctr, "counter_add: bad args");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ctr, delta);
  MR_CHECK_LAUNCH("counter_add");
  return MRMT3_OK;
}

extern "C" size_t mrmt3_opt_ranges_table_bytes(int n_ranges) {
  return n_ranges < 0 ? 0 : ((size_t)n_ranges + 1) * sizeof(MrOptRec);
}

extern "C" int mrmt3_opt_ranges_plan(const mrmt3_opt_range* ranges, int n_ranges, size_t n, void* table_host,
                                     size_t table_bytes, size_t* n_trainable) {
  MR_CHECK_ARG(ranges && table_host, "opt_ranges_plan: null pointer");
  MR_CHECK_ARG(n_ranges >= 1 && n_ranges <= MR_OPT_MAX_RANGES, "opt_ranges_plan: %d ranges (1 .. %d: freezing everything leaves nothing to step)",
               n_ranges, MR_OPT_MAX_RANGES);
  MR_CHECK_ARG(n > 0 && n % 4 == 0, "opt_ranges_plan: n = %zu must be a positive multiple of 4", n);
  MR_CHECK_ARG(table_bytes >= mrmt3_opt_ranges_table_bytes(n_ranges), "opt_ranges_plan: the table holds %zu bytes, %zu are needed",
               table_bytes, mrmt3_opt_ranges_table_bytes(n_ranges));
  int bad = 0;
  const char* why = mr_opt_ranges_problem(ranges, n_ranges, n, &bad);
  MR_CHECK_ARG(why[0] == 0, "opt_ranges_plan: range %d [%lld, %lld): %s", bad, ranges[bad].begin, ranges[bad].end, why);
  const size_t tr = mr_opt_ranges_fill(ranges, n_ranges, (MrOptRec*)table_host);
  if (n_trainable) *n_trainable = tr;
  return MRMT3_OK;
}

extern "C" int mrmt3_adamw_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, const void* ranges_dev,
                                int n_ranges, size_t n_trainable, const float* lr_dev, int32_t* step_dev, float beta1,
                                float beta2, float eps, float weight_decay, float grad_scale, float ema_decay,
                                const float* stat_dev, float clip_value, void* shadow_bf16, void* stream) {
  MR_CHECK_ARG(p && g && m && v && lr_dev && step_dev && n % 4 == 0, "adamw_step: bad args");
  MR_CHECK_ARG((ranges_dev != nullptr) == (n_ranges != 0),
               "adamw_step: bad args: ranges_dev and n_ranges come together (NULL and 0: the flat form), got %s and %d ranges",
               ranges_dev ? "a table" : "NULL", n_ranges);
  MR_CHECK_ARG(clip_value >= 0.f, "adamw_step: clip_value = %g is negative (0: no clamp)", (double)clip_value);
  MR_CHECK_ARG(stat_dev || clip_value == 0.f, "adamw_step: clip_value needs stat_dev (the clipped form)");
  // ema_decay == 0 means "no EMA" and needs ema == null; otherwise 0 < ema_decay < 1 and a buffer
  MR_CHECK_ARG(ema_decay == 0.f || (ema_decay > 0.f && ema_decay < 1.f), "adamw_step: ema_decay = %g is outside (0, 1)",
               (double)ema_decay);
  MR_CHECK_ARG((ema != nullptr) == (ema_decay != 0.f), "adamw_step: ema_decay = %g %s", (double)ema_decay,
               ema ? "but an ema buffer was given (0 < ema_decay < 1 is needed)" : "needs an ema buffer (null was given)");
  hipStream_t s = (hipStream_t)stream;
  bf16_t* shadow = (bf16_t*)shadow_bf16;
  if (!ranges_dev) {
    MR_CHECK_ARG(!ema, "adamw_step: the flat form keeps no EMA (an ema buffer needs a range table)");
    const dim3 grid(ew_blocks(n / 4)), block(256);
#define AW_LAUNCH(C_)                                                                                                  \
  hipLaunchKernelGGL(adamw_kernel<C_>, grid, block, 0, s, p, g, m, v, n / 4, lr_dev, step_dev, beta1, beta2, eps,       \
                     weight_decay, grad_scale, stat_dev, clip_value, shadow)
    if (stat_dev) AW_LAUNCH(true); else AW_LAUNCH(false);
#undef AW_LAUNCH
  } else {
    MR_CHECK_ARG(n_ranges >= 1 && n_ranges <= MR_OPT_MAX_RANGES, "adamw_step: %d ranges (1 .. %d)", n_ranges, MR_OPT_MAX_RANGES);
    MR_CHECK_ARG(n_trainable > 0 && n_trainable % 4 == 0 && n_trainable <= n,
                 "adamw_step: n_trainable = %zu must be a positive multiple of 4, at most n = %zu", n_trainable, n);
    MR_CHECK_ARG(((uintptr_t)ranges_dev & 7) == 0, "adamw_step: the range table must be 8-byte aligned");
    const size_t groups = n_trainable / 4;
    const dim3 grid((unsigned)((groups + OG_CHUNK - 1) / OG_CHUNK)), block(256);
    const MrOptRec* tab = (const MrOptRec*)ranges_dev;
    const float om = 1.f - ema_decay;
#define OG_LAUNCH(C_, E_)                                                                                              \
  hipLaunchKernelGGL((adamw_groups_kernel<C_, E_>), grid, block, 0, s, p, g, m, v, ema, tab, n_ranges, lr_dev, step_dev, \
                     beta1, beta2, eps, grad_scale, om, stat_dev, clip_value, shadow)
    if (stat_dev) { if (ema) OG_LAUNCH(true, true); else OG_LAUNCH(true, false); }
    else          { if (ema) OG_LAUNCH(false, true); else OG_LAUNCH(false, false); }
#undef OG_LAUNCH
  }
  MR_CHECK_LAUNCH("adamw_step");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, s, step_dev, 1);
  MR_CHECK_LAUNCH("adamw_step inc");
  return MRMT3_OK;
}

// ------------------------------------------------------------------------------------------------
// Global gradient norm + clip coefficient + non-finite guard
// ------------------------------------------------------------------------------------------------
// Stage 1 runs a FIXED grid whatever the device and n: the order of every addition is a function of n (RANGES: of the
// table) alone, so every rank and every box lands on the same bits.  2048 workgroups x 4 waves = 32 waves per CU on 256
// CUs, 4 x 16 B in flight per lane.  g*g is exact in f64 (24 x 24 significand bits), so the only roundings are the f64
// additions.
#define GN_BLOCKS 2048
#define GN_PER_LANE (GN_BLOCKS / 256)      // partials per lane of stage 2

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the 256 threads of a workgroup, valid in thread 0: the wave's xor tree, then the 4 waves in index order
__device__ __forceinline__ double block_sum_f64(double v, double* lds4) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

__device__ __forceinline__ void sumsq4_f64(const float gv[4], double acc[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double d = (double)gv[e];
    acc[e] += d * d;
  }
}

// group i of g; RANGES: group i of the virtual array of the ranges (the indices of a lane only grow: each search starts
// at the last hit, r)
template <bool RANGES>
__device__ __forceinline__ void gn_load4(const float* __restrict__ g, const MrOptRec* __restrict__ tab, int nr, int& r,
                                         long long i, float out[4]) {
  if (RANGES) {
    r = opt_locate(tab, r, nr, i);
    i = tab[r].begin4 + (i - tab[r].start);
  }
  load4<float>(g + (size_t)i * 4, out);
}

// n4 groups (RANGES: the table's total).  With ONE range covering the buffer the two forms add in the same order: the
// same bits.
template <bool RANGES>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n4,
                                                         const MrOptRec* __restrict__ tab, int nr,
                                                         double* __restrict__ partial) {
  __shared__ double lds4[4];
  if (RANGES) n4 = tab[nr].start;
  const long long stride = (long long)GN_BLOCKS * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int r = 0;
  for (; i + 3 * stride < n4; i += 4 * stride) {             // four independent 16-byte loads in flight per lane
    float a[4], b[4], c[4], d[4];
    gn_load4<RANGES>(g, tab, nr, r, i, a);
    gn_load4<RANGES>(g, tab, nr, r, i + stride, b);
    gn_load4<RANGES>(g, tab, nr, r, i + 2 * stride, c);
    gn_load4<RANGES>(g, tab, nr, r, i + 3 * stride, d);
    sumsq4_f64(a, acc); sumsq4_f64(b, acc); sumsq4_f64(c, acc); sumsq4_f64(d, acc);
  }
  for (; i < n4; i += stride) {
    float a[4];
    gn_load4<RANGES>(g, tab, nr, r, i, a);
    sumsq4_f64(a, acc);
  }
  const double s = block_sum_f64((acc[0] + acc[1]) + (acc[2] + acc[3]), lds4);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Stage 2, one workgroup: lane t sums partials [t*8, t*8+8) in index order, then the same fixed tree as stage 1.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, float grad_scale,
                                                               float max_norm, int skip_nonfinite,
                                                               float* __restrict__ stat, int32_t* __restrict__ skipped) {
  __shared__ double lds4[4];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < GN_PER_LANE; ++k) s += partial[threadIdx.x * GN_PER_LANE + k];
  s = block_sum_f64(s, lds4);
  if (threadIdx.x != 0) return;
  const float norm = (float)(sqrt(s) * (double)grad_scale);
  float coef = 1.f;
  if (max_norm > 0.f) {
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.f ? 1.f : c;                               // clamp(max=1): a NaN stays a NaN, like torch's
  }
  float skip = 0.f;
  if (skip_nonfinite && !(fabsf(norm) <= 3.402823466e38f)) {   // inf or NaN
    skip = 1.f;
    coef = 0.f;
    skipped[0] += 1;
  }
  stat[0] = norm;
  stat[1] = coef;
  stat[2] = skip;
}

extern "C" size_t mrmt3_grad_norm_workspace_elems(void) { return (size_t)GN_BLOCKS * 2; }   // one f64 per workgroup

extern "C" int mrmt3_grad_norm(const float* g, size_t n, const void* ranges_dev, int n_ranges, float grad_scale,
                               float max_norm, int skip_nonfinite, float* ws, size_t ws_elems, float* stat_dev,
                               int32_t* skipped_dev, void* stream) {
  MR_CHECK_ARG(g && ws && stat_dev && skipped_dev, "grad_norm: null pointer");
  MR_CHECK_ARG(n > 0 && n % 4 == 0 && ((uintptr_t)g & 15) == 0, "grad_norm: n = %zu must be a positive multiple of 4 and g 16-byte aligned", n);
  MR_CHECK_ARG((ranges_dev != nullptr) == (n_ranges != 0),
               "grad_norm: ranges_dev and n_ranges come together (a null pointer and 0 ranges: all of g), got %s and %d ranges",
               ranges_dev ? "a table" : "a null pointer", n_ranges);
  MR_CHECK_ARG(!ranges_dev || (n_ranges >= 1 && n_ranges <= MR_OPT_MAX_RANGES), "grad_norm: %d ranges (1 .. %d)", n_ranges, MR_OPT_MAX_RANGES);
  MR_CHECK_ARG(((uintptr_t)ranges_dev & 7) == 0, "grad_norm: the range table must be 8-byte aligned");
  MR_CHECK_ARG(ws_elems >= mrmt3_grad_norm_workspace_elems() && ((uintptr_t)ws & 7) == 0,
               "grad_norm: the workspace holds %zu floats, %zu are needed (8-byte aligned)", ws_elems,
               mrmt3_grad_norm_workspace_elems());
  MR_CHECK_ARG(max_norm >= 0.f, "grad_norm: max_norm = %g is negative (0: no clipping)", (double)max_norm);
  hipStream_t s = (hipStream_t)stream;
  const MrOptRec* tab = (const MrOptRec*)ranges_dev;
  if (tab) hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(GN_BLOCKS), dim3(256), 0, s, g, 0LL, tab, n_ranges, (double*)ws);
  else hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(GN_BLOCKS), dim3(256), 0, s, g, (long long)(n / 4), tab, 0, (double*)ws);
  MR_CHECK_LAUNCH("grad_norm");
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, grad_scale, max_norm,
                     skip_nonfinite, stat_dev, skipped_dev);
  MR_CHECK_LAUNCH("grad_norm finish");
  return MRMT3_OK;
}

