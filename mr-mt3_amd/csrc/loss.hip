// The loss: cross-entropy (plain, and with label smoothing + z-loss), teacher-forced token scoring, and the lm_head
// drivers that run the lm_head product and one of those row kernels chunk by chunk, so that the [rows][V] f32 logits never
// exist whole.
#include "common.h"
#include "rowmath.h"

// no implicit FMA formation in this file: the log-sum-exp chains, the regularised objective and the gradient scaling of
// ce_kernel / ce_wave_kernel and the (l[target] - max) - log(sum) of token_logprob_kernel have their bits pinned under
// this setting
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// cross-entropy (tasks/mt3_net.py:32-35; weighted variant tasks/mt3_net.py:96-108)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ce_weights(int64_t t, int weighted, int lo, int hi, float* w, float* n) {
  if (t == -100) { *w = 0.f; *n = 0.f; return; }
  if (weighted && t >= lo && t <= hi) { *w = 3.f; *n = 2.f; return; }
  *w = 1.f; *n = 1.f;
}

__global__ void ce_count_kernel(const int64_t* __restrict__ targets, int rows, int weighted, int lo, int hi,
                                float* __restrict__ denom) {
  float s = 0.f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += gridDim.x * blockDim.x) {
    float w, n;
    ce_weights(targets[i], weighted, lo, hi, &w, &n);
    s += n;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0 && s != 0.f) atomicAdd(denom, s);
}

extern "C" int mrmt3_ce_count(const int64_t* targets, int rows, int weighted, int inst_lo, int inst_hi,
                              float* denom_dev, void* stream) {
  MR_CHECK_ARG(targets && denom_dev && rows > 0, "ce_count: bad args");
  int blocks = ceil_div(rows, 256);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(ce_count_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, targets, rows, weighted,
                     inst_lo, inst_hi, denom_dev);
  MR_CHECK_LAUNCH("ce_count");
  return MRMT3_OK;
}

// REG (label smoothing eps + z-loss z): per scored row r = (1-eps)*nll + eps*(lse - mean_j l[j]) + z*lse^2;
// loss[0] receives the objective sum_i w_i r_i / denom, loss[1] the plain NLL, and the gradient is
// gs * (p_j*(1 + 2 z lse) - (1-eps)[j==t] - eps/V).  REG = false is the kernel of before, statement for statement: eps
// and z are then never read and loss[1] never written.
template <typename TD, bool REG>
__global__ __launch_bounds__(256) void ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                 const float* __restrict__ denom, double* __restrict__ loss,
                                                 TD* __restrict__ dlogits, int rows, int V, int weighted, int lo,
                                                 int hi, float grad_scale, float eps, float z) {
  __shared__ float red[REG ? 12 : 8];
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lp = logits + (size_t)row * V;
  const int64_t t = targets[row];
  float w, n;
  ce_weights(t, weighted, lo, hi, &w, &n);
  TD* dp = dlogits ? dlogits + (size_t)row * V : nullptr;
  if (w == 0.f) {
    if (dp) for (int c = tid * 4; c < V; c += 1024) { float z4[4] = {0.f, 0.f, 0.f, 0.f}; store4<TD>(dp + c, z4); }
    return;
  }
  // one pass over the row: running (max, sum of exp) per thread, merged across the workgroup (REG: and the running sum
  // of the raw logits next to them)
  float mx = -INFINITY, se = 0.f, sm = 0.f;
  for (int c = tid * 4; c < V; c += 1024) {
    float v[4];
    load4<float>(lp + c, v);
    const float m4 = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    const float mn = fmaxf(mx, m4);
    se = se * expf(mx - mn) + ((expf(v[0] - mn) + expf(v[1] - mn)) + (expf(v[2] - mn) + expf(v[3] - mn)));
    mx = mn;
    if constexpr (REG) sm += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float wmx = wave_max(mx);
  se = wave_sum(mx == -INFINITY ? 0.f : se * expf(mx - wmx));
  if constexpr (REG) sm = wave_sum(sm);
  if (lane == 0) {
    red[wave] = wmx;
    red[4 + wave] = se;
    if constexpr (REG) red[8 + wave] = sm;
  }
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  se = 0.f;
#pragma unroll
  for (int w4 = 0; w4 < 4; ++w4) se += red[4 + w4] * expf(red[w4] - mx);
  const float lse = mx + logf(se);
  const float inv_den = 1.f / denom[0];
  if constexpr (REG) {
    if (tid == 0) {
      const float nll = lse - lp[t];
      const float u = lse - ((red[8] + red[9]) + (red[10] + red[11])) * (1.f / (float)V);
      const float r = (1.f - eps) * nll + eps * u + z * lse * lse;
      atomicAdd(loss, (double)(w * r * inv_den));
      atomicAdd(loss + 1, (double)(w * nll * inv_den));
    }
  } else {
    if (tid == 0) atomicAdd(loss, (double)(w * (lse - lp[t]) * inv_den));
  }
  if (dp) {
    const float gs = w * inv_den * grad_scale;
    const float pz = REG ? 1.f + 2.f * z * lse : 1.f;           // d(lse + z lse^2)/d lse
    const float hot = REG ? 1.f - eps : 1.f, uni = REG ? eps / (float)V : 0.f;
    for (int c = tid * 4; c < V; c += 1024) {
      float v[4];
      load4<float>(lp + c, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float p = expf(v[e] - lse);
        if constexpr (REG) {
          p = p * pz - uni;
          if (c + e == t) p -= hot;
        } else {
          if (c + e == t) p -= 1.f;
        }
        v[e] = p * gs;
      }
      store4<TD>(dp + c, v);
    }
  }
}

// fast path for V = NV*256 <= 2048 (MT3: 1536): one WAVE per row, the row lives in registers (one
// HBM read), statistics by wave shuffles.  A wave walks CE_RPW consecutive rows and the workgroup adds its
// loss contribution with ONE atomic: one atomic per row (65 536 of them on a single address) cost more
// than the whole rest of the kernel.
// Rows per wave: as few as keep the launch at ~2048 workgroups (a wave walks its rows one after the other, each a
// load -> max -> exp -> sum -> store chain of ~3.5 us: at 16 rows per wave a 16 384-row chunk ran 4 waves per CU and
// 2.6 TB/s; at 2 rows per wave the CUs are full), at most 16.
static inline int ce_rows_per_wave(int rows) {
  int r = rows / (4 * 2048);
  return r < 1 ? 1 : (r > 16 ? 16 : r);
}
// REG as in ce_kernel: the row sum of the raw logits is one more per-lane partial of the load pass and one more wave_sum;
// the workgroup adds two scalars (objective, NLL) instead of one.
template <typename TD, int NV, bool REG>
__global__ __launch_bounds__(256) void ce_wave_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                      const float* __restrict__ denom, double* __restrict__ loss,
                                                      TD* __restrict__ dlogits, int rows, int weighted, int lo, int hi,
                                                      float grad_scale, int rpw, float eps, float z) {
  constexpr int V = NV * 256;
  __shared__ float part[REG ? 8 : 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = (blockIdx.x * 4 + wave) * rpw;
  const float inv_den = 1.f / denom[0];
  float acc = 0.f, acc_nll = 0.f;
  for (int row = row0; row < min(row0 + rpw, rows); ++row) {
    const float* lp = logits + (size_t)row * V;
    const int64_t t = targets[row];
    float w, n;
    ce_weights(t, weighted, lo, hi, &w, &n);
    TD* dp = dlogits ? dlogits + (size_t)row * V : nullptr;
    if (w == 0.f) {
      if (dp) {
        const float z4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NV; ++i) store4<TD>(dp + (i * 64 + lane) * 4, z4);
      }
      continue;
    }
    float v[NV][4];
    float mx = -INFINITY, sm = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      load4<float>(lp + (i * 64 + lane) * 4, v[i]);
      mx = fmaxf(mx, fmaxf(fmaxf(v[i][0], v[i][1]), fmaxf(v[i][2], v[i][3])));
      if constexpr (REG) sm += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float zt = lp[t];
    mx = wave_max(mx);
    if constexpr (REG) sm = wave_sum(sm);
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[i][e] = expf(v[i][e] - mx);
        se += v[i][e];
      }
    se = wave_sum(se);
    const float lse = mx + logf(se);
    if constexpr (REG) {
      const float nll = lse - zt;
      const float u = lse - sm * (1.f / (float)V);
      acc += w * ((1.f - eps) * nll + eps * u + z * lse * lse) * inv_den;
      acc_nll += w * nll * inv_den;
    } else {
      acc += w * (lse - zt) * inv_den;
    }
    if (dp) {
      if constexpr (REG) {
        const float g0 = w * inv_den * grad_scale;
        const float gs = g0 * (1.f + 2.f * z * lse) / se;        // v * gs = g0 * p_j * (1 + 2 z lse)
        const float hot = g0 * (1.f - eps), uni = g0 * (eps / (float)V);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int c = (i * 64 + lane) * 4;
          float g[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] = (v[i][e] * gs - uni) - ((c + e == t) ? hot : 0.f);
          store4<TD>(dp + c, g);
        }
      } else {
        const float gs = w * inv_den * grad_scale / se;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int c = (i * 64 + lane) * 4;
          float g[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] = v[i][e] * gs - ((c + e == t) ? w * inv_den * grad_scale : 0.f);
          store4<TD>(dp + c, g);
        }
      }
    }
  }
  if (lane == 0) {
    part[wave] = acc;
    if constexpr (REG) part[4 + wave] = acc_nll;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // the loss scalar is a DOUBLE: the order in which the workgroups' sums arrive perturbs it at 1e-16, far below the
    // f32 value that is logged — two runs log the same float (a float accumulator wandered by a few ulp per run)
    const double tot = ((double)part[0] + (double)part[1]) + ((double)part[2] + (double)part[3]);
    if (tot != 0.0) atomicAdd(loss, tot);
    if constexpr (REG) {
      const double nll = ((double)part[4] + (double)part[5]) + ((double)part[6] + (double)part[7]);
      if (nll != 0.0) atomicAdd(loss + 1, nll);
    }
  }
}

template <bool REG>
static int ce_launch(const float* logits, const int64_t* targets, const float* denom_dev, double* loss_dev, void* dlogits,
                     int dl_dtype, int rows, int V, int weighted, int inst_lo, int inst_hi, float grad_scale, float eps,
                     float z, hipStream_t s, const char* name) {
  MR_CHECK_DTYPE(name, dl_dtype);
  mr_dtype(dl_dtype, [&](auto td) {
    using TD = typename decltype(td)::type;
    // V = 512, 1024, 1536, 2048: the wave kernel; any other V: the general one
    const bool wave = mr_const<2, 4, 6, 8>(V % 256 ? 0 : V / 256, [&](auto nv) {
      const int rpw = ce_rows_per_wave(rows);
      hipLaunchKernelGGL((ce_wave_kernel<TD, decltype(nv)::value, REG>), dim3((unsigned)ceil_div(rows, 4 * rpw)), dim3(256), 0,
                         s, logits, targets, denom_dev, loss_dev, (TD*)dlogits, rows, weighted, inst_lo, inst_hi, grad_scale,
                         rpw, eps, z);
    });
    if (!wave)
      hipLaunchKernelGGL((ce_kernel<TD, REG>), dim3(rows), dim3(256), 0, s, logits, targets, denom_dev, loss_dev,
                         (TD*)dlogits, rows, V, weighted, inst_lo, inst_hi, grad_scale, eps, z);
  });
  MR_CHECK_LAUNCH(name);
  return MRMT3_OK;
}

extern "C" int mrmt3_ce_fwd_bwd(const float* logits, const int64_t* targets, const float* denom_dev, double* loss_dev,
                                void* dlogits, int dl_dtype, int rows, int V, int weighted, int inst_lo,
                                int inst_hi, float grad_scale, void* stream) {
  MR_CHECK_ARG(logits && targets && denom_dev && loss_dev && rows > 0 && V % 4 == 0, "ce_fwd_bwd: bad args");
  return ce_launch<false>(logits, targets, denom_dev, loss_dev, dlogits, dl_dtype, rows, V, weighted, inst_lo, inst_hi,
                          grad_scale, 0.f, 0.f, (hipStream_t)stream, "ce_fwd_bwd");
}

extern "C" int mrmt3_ce_fwd_bwd_reg(const float* logits, const int64_t* targets, const float* denom_dev, float label_smoothing,
                                    float z_loss, double* loss_dev, void* dlogits, int dl_dtype, int rows, int V,
                                    int weighted, int inst_lo, int inst_hi, float grad_scale, void* stream) {
  MR_CHECK_CE_OPTIONS("ce_fwd_bwd_reg", label_smoothing, z_loss);
  MR_CHECK_ARG(logits && targets && denom_dev && loss_dev && rows > 0 && V > 0 && V % 4 == 0, "ce_fwd_bwd_reg: bad args");
  return ce_launch<true>(logits, targets, denom_dev, loss_dev, dlogits, dl_dtype, rows, V, weighted, inst_lo, inst_hi,
                         grad_scale, label_smoothing, z_loss, (hipStream_t)stream, "ce_fwd_bwd_reg");
}

// ------------------------------------------------------------------------------------------------
// log-probability of one target per row (teacher-forced scoring; forward only).  One wave per row; the row (up to
// 64 * TLP_REGS logits; longer rows are refused) stays in registers, so it is read once.  Same arithmetic and
// summation order as the greedy decoder's tail (decode_tail.hip dec_argmax<., true>): NaN-propagating maximum, exp(l - max)
// summed per lane in ascending column then the xor tree, (l[target] - max) - log(sum).
// ------------------------------------------------------------------------------------------------
#define TLP_REGS 32
__global__ __launch_bounds__(256) void token_logprob_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                            float* __restrict__ out, int rows, int V, int ignore_index) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t t = targets[row];
  if (t == ignore_index || t < 0 || t >= V) {
    if (lane == 0) out[row] = (t == ignore_index) ? 0.f : __int_as_float(0x7fc00000);   // a target outside [0, V): NaN
    return;
  }
  const float* lp = logits + (size_t)row * V;
  float v[TLP_REGS];
  float mx = -INFINITY, se = 0.f;
#pragma unroll
  for (int i = 0; i < TLP_REGS; ++i) {
    const int c = lane + 64 * i;
    v[i] = (c < V) ? lp[c] : -INFINITY;
  }
#pragma unroll
  for (int i = 0; i < TLP_REGS; ++i) mx = nanmax(mx, v[i]);
  mx = wave_nanmax(mx);
#pragma unroll
  for (int i = 0; i < TLP_REGS; ++i) se += expf(v[i] - mx);        // columns past V are -inf: 0
  se = wave_sum(se);
  if (lane == 0) out[row] = (lp[t] - mx) - logf(se);
}

extern "C" int mrmt3_token_logprob(const float* logits, const int64_t* targets, float* out, int rows, int V,
                                   int ignore_index, void* stream) {
  MR_CHECK_ARG(logits && targets && out && rows > 0 && V > 0, "token_logprob: bad args");
  MR_CHECK_ARG(V <= 64 * TLP_REGS, "token_logprob: vocab %d exceeds the %d logits a wave keeps in registers", V, 64 * TLP_REGS);
  const dim3 grid((unsigned)ceil_div(rows, 4)), block(256);
  hipLaunchKernelGGL(token_logprob_kernel, grid, block, 0, (hipStream_t)stream, logits, targets, out, rows, V, ignore_index);
  MR_CHECK_LAUNCH("token_logprob");
  return MRMT3_OK;
}

// ------------------------------------------------------------------------------------------------
// lm_head projection + a row kernel without the [rows][V] f32 logits in memory.
//
// Reference: `lm_logits = self.lm_head(sequence_output)` (models/t5.py:72,176-180) followed by
// `CrossEntropyLoss(ignore_index=-100)(lm_logits.view(-1, V), targets.view(-1))` (tasks/mt3_net.py:32-35): at the benchmark
// batch that is a [65536][1536] f32 tensor — 403 MB written by the GEMM, read back by the loss, and kept alive until the
// backward.  Here the rows are processed in chunks: the GEMM of a chunk writes its logits into a workspace that is reused
// (and, at 50-100 MB, stays in the 256 MB Infinity Cache), the loss kernel reads it there, adds the chunk's share of the
// loss and leaves only the bf16 gradient w.r.t. the logits, which the two backward GEMMs of lm_head consume.
// Arithmetic per row is exactly mrmt3_gemm_nt + mrmt3_ce_fwd_bwd (same kernels), so loss and gradients equal the unfused
// path bit for bit; the loss scalar is accumulated in double (atomic adds in arrival order: 1e-16, invisible in the logged float).
// ------------------------------------------------------------------------------------------------
// The one chunk loop: dec [rows][ld_dec] and W [V][ldw] of `dtype`; `step(logits, r0, n)` consumes the f32 logits of rows
// [r0, r0 + n) from the workspace.  `others`: the entry point's own pointers are all non-null.
template <typename Step>
static int lmhead_chunks(const char* who, const void* dec, int ld_dec, const void* W, int ldw, int dtype, bool others,
                         int rows, int V, int d, void* workspace, size_t workspace_bytes, int chunk_rows, void* stream,
                         Step&& step) {
  MR_CHECK_ARG(dec && W && workspace && others, "%s: null pointer", who);
  MR_CHECK_ARG(rows > 0 && V > 0 && d > 0 && chunk_rows > 0, "%s: bad sizes", who);
  MR_CHECK_ARG(workspace_bytes >= (size_t)(chunk_rows < rows ? chunk_rows : rows) * V * sizeof(float),
               "%s: workspace smaller than one chunk of logits", who);
  for (int r0 = 0; r0 < rows; r0 += chunk_rows) {
    const int n = rows - r0 < chunk_rows ? rows - r0 : chunk_rows;
    int rc = mrmt3_gemm_nt((const char*)dec + (size_t)r0 * ld_dec * mr_dtype_bytes(dtype), ld_dec, W, ldw, workspace, V, n, V,
                           d, dtype, MRMT3_F32, 0, stream);
    if (rc == MRMT3_OK) rc = step((const float*)workspace, r0, n);
    if (rc != MRMT3_OK) return rc;
  }
  return MRMT3_OK;
}
// rows r0.. of the logits gradient (null stays null)
static inline void* dl_rows(void* dlogits, int dl_dtype, int r0, int V) {
  return dlogits ? (char*)dlogits + (size_t)r0 * V * mr_dtype_bytes(dl_dtype) : nullptr;
}

extern "C" int mrmt3_lmhead_ce_fwd_bwd(const void* dec, int ld_dec, const void* W, int ldw, const int64_t* targets,
                                       const float* denom_dev, double* loss_dev, void* dlogits, int dl_dtype, int rows,
                                       int V, int d, int weighted, int inst_lo, int inst_hi, float grad_scale,
                                       void* workspace, size_t workspace_bytes, int chunk_rows, void* stream) {
  MR_CHECK_DTYPE("lmhead_ce", dl_dtype);
  return lmhead_chunks("lmhead_ce", dec, ld_dec, W, ldw, MRMT3_BF16, targets && denom_dev && loss_dev, rows, V, d, workspace,
                       workspace_bytes, chunk_rows, stream, [&](const float* logits, int r0, int n) {
    return mrmt3_ce_fwd_bwd(logits, targets + r0, denom_dev, loss_dev, dl_rows(dlogits, dl_dtype, r0, V), dl_dtype, n, V,
                            weighted, inst_lo, inst_hi, grad_scale, stream);
  });
}

// The same with mrmt3_ce_fwd_bwd_reg (label smoothing + z-loss): loss_dev[0] accumulates the objective, loss_dev[1] the
// plain NLL.
extern "C" int mrmt3_lmhead_ce_fwd_bwd_reg(const void* dec, int ld_dec, const void* W, int ldw, const int64_t* targets,
                                           const float* denom_dev, float label_smoothing, float z_loss, double* loss_dev,
                                           void* dlogits, int dl_dtype, int rows, int V, int d, int weighted, int inst_lo,
                                           int inst_hi, float grad_scale, void* workspace, size_t workspace_bytes,
                                           int chunk_rows, void* stream) {
  MR_CHECK_CE_OPTIONS("lmhead_ce_reg", label_smoothing, z_loss);
  MR_CHECK_DTYPE("lmhead_ce_reg", dl_dtype);
  return lmhead_chunks("lmhead_ce_reg", dec, ld_dec, W, ldw, MRMT3_BF16, targets && denom_dev && loss_dev, rows, V, d,
                       workspace, workspace_bytes, chunk_rows, stream, [&](const float* logits, int r0, int n) {
    return mrmt3_ce_fwd_bwd_reg(logits, targets + r0, denom_dev, label_smoothing, z_loss, loss_dev,
                                dl_rows(dlogits, dl_dtype, r0, V), dl_dtype, n, V, weighted, inst_lo, inst_hi, grad_scale, stream);
  });
}

// Teacher-forced scoring: out[r] = log p(targets[r]) under softmax(dec[r] . W^T), 0 where the target is -100.  The same
// with mrmt3_token_logprob in place of the loss kernel; forward only, operands bf16 or f32 (`dtype`).
extern "C" int mrmt3_lmhead_logprob(const void* dec, int ld_dec, const void* W, int ldw, const int64_t* targets, float* out,
                                    int rows, int V, int d, int dtype, void* workspace, size_t workspace_bytes,
                                    int chunk_rows, void* stream) {
  MR_CHECK_DTYPE("lmhead_logprob", dtype);
  return lmhead_chunks("lmhead_logprob", dec, ld_dec, W, ldw, dtype, targets && out, rows, V, d, workspace, workspace_bytes,
                       chunk_rows, stream, [&](const float* logits, int r0, int n) {
    return mrmt3_token_logprob(logits, targets + r0, out + r0, n, V, -100, stream);
  });
}

