// The HBM-bound row kernels of the T5 block: fused residual-add + dropout + T5LayerNorm (RMS) forward and backward, the
// norm-weight partial rows and their reduce, gated-GELU forward and backward.  These are the stand-alone forms of the
// rowmath.h arithmetic that gemm_rows.hip fuses into its projections.  (The other row-wise sources: embed.hip, loss.hip,
// optim.hip, layout.hip.)
//
// All of them stream their rows once with 16-byte accesses (float4 / 8 x bf16 per lane), keep the
// row statistics in fp32 and reduce with 64-lane wave shuffles.
#include "common.h"
#include "rowmath.h"

// no implicit FMA formation in this file: the norm and gated-GELU arithmetic is rowmath.h's, which switches contraction off
// per function; what the kernels here add around it (the dw partial sums) holds no product today, so this pins whatever
// joins them later to the bits of the fused forms in gemm_rows.hip, which is compiled under the same setting
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// fused add + dropout + RMS norm, forward.   one wave per row, 4 rows per workgroup
// HF T5LayerNorm: w * (x * rsqrt(mean(x^2) + eps)), fp32 statistics.
// ------------------------------------------------------------------------------------------------
#define NORM_MAXV 8  // float4 groups per lane: cols <= 64*4*8 = 2048

template <typename TY, typename TN, int NV>
__global__ __launch_bounds__(256) void add_rmsnorm_fwd_kernel(const float* __restrict__ x0, const TY* __restrict__ y,
                                                              const float* __restrict__ w, float eps,
                                                              float* __restrict__ x1, TN* __restrict__ xn,
                                                              float* __restrict__ rstd_out, int rows, int cols,
                                                              DropCfg dy, DropCfg dout, int out_drop, int cache_mode) {
  DROP_STEP(dy); DROP_STEP(dout);
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  constexpr int nv = NV;  // float4 groups per lane (cols = NV*256)
  float v[NV][4];
  float ss = 0.f;
  const size_t base = (size_t)row * cols;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (i < nv) {
      const int col = i * 256 + lane * 4;
      if (cache_mode & 2) load4_nt<float>(x0 + base + col, v[i]);
      else load4<float>(x0 + base + col, v[i]);
      if (y != nullptr) {
        float yv[4];
        load4<TY>(y + base + col, yv);
        norm_fwd_add(dy, (base + col) >> 2, v[i], yv);
      }
      if (x1 != nullptr) {
        if (cache_mode & 1) store4_nt<float>(x1 + base + col, v[i]);
        else store4<float>(x1 + base + col, v[i]);
      }
      ss = norm_fwd_sumsq(v[i], ss);
    }
  }
  const float rstd = norm_rstd(wave_sum(ss), (float)cols, eps);
  if (lane == 0 && rstd_out != nullptr) rstd_out[row] = rstd;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (i < nv) {
      const int col = i * 256 + lane * 4;
      float wv[4], o[4];
      load4<float>(w + col, wv);
      norm_fwd_out(wv, v[i], rstd, dout, out_drop, (base + col) >> 2, o);
      store4<TN>(xn + base + col, o);
    }
  }
}

extern "C" int mrmt3_add_rmsnorm_fwd(const float* x0, const void* y, int y_dtype, const float* w, float eps,
                                     float* x1, void* xn, int xn_dtype, float* rstd, int rows, int cols,
                                     float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_y, uint32_t stream_out,
                                     int out_drop, void* stream) {
  MR_CHECK_ARG(x0 && w && xn, "add_rmsnorm_fwd: null pointer");
  MR_CHECK_ARG(rows > 0 && (cols == 256 || cols == 512 || cols == 1024 || cols == 2048),
               "add_rmsnorm_fwd: cols must be 256, 512, 1024 or 2048");
  MR_CHECK_DTYPE("add_rmsnorm_fwd", y_dtype);
  MR_CHECK_DTYPE("add_rmsnorm_fwd", xn_dtype);
  DropCfg dy = make_drop(p_drop, seed, stream_y, step_dev), dn = make_drop(p_drop, seed, stream_out, step_dev);
  dim3 grid((unsigned)ceil_div(rows, 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  // bit 0: streaming store of the residual stream x1 (its reader is the next norm, three kernels on), bit 1: streaming
  // load of x0.  64 segments, same box, three alternations: 0 26.00 ms, 1 25.81, 2 25.97, 3 25.79 (MRMT3_NORM_NT)
  const int cache_mode = MR_KNOB("MRMT3_NORM_NT", 3);
  mr_dtype(y_dtype, [&](auto ty) {
    mr_dtype(xn_dtype, [&](auto tn) {
      mr_const<1, 2, 4, 8>(cols / 256, [&](auto nv) {
        using TY = typename decltype(ty)::type;
        using TN = typename decltype(tn)::type;
        hipLaunchKernelGGL((add_rmsnorm_fwd_kernel<TY, TN, decltype(nv)::value>), grid, block, 0, s, x0, (const TY*)y, w,
                           eps, x1, (TN*)xn, rstd, rows, cols, dy, dn, out_drop, cache_mode);
      });
    });
  });
  MR_CHECK_LAUNCH("add_rmsnorm_fwd");
  return MRMT3_OK;
}

// backward: each workgroup owns NB_ROWS consecutive rows (wave w takes rows w, w+4, ...), keeps the
// per-column dw partial sums in registers and issues one f32 atomic per column at the end.
// rows per workgroup: 32 for the tall decoder shapes (2048 workgroups at 65536 rows), fewer for shorter inputs so that
// a launch still has >= ~2048 workgroups (12 segments per GPU: 12288 rows ran 384 workgroups at 3.1 TB/s of 6-7)
static inline int nb_rows(int rows) {
  int r = 32;
  while (r > 4 && rows / r < 2048) r >>= 1;
  return r;
}
template <int NV, typename TG, typename TRI, typename TRO>
__global__ __launch_bounds__(256) void add_rmsnorm_bwd_kernel(const TG* __restrict__ dxn, const TRI* __restrict__ dres,
                                                              const float* __restrict__ x1, const float* __restrict__ rstd_in,
                                                              const float* __restrict__ w, TRO* __restrict__ dx1,
                                                              bf16_t* __restrict__ dy, float* __restrict__ dw_part, int rows,
                                                              int cols, DropCfg ddy, DropCfg dout, int out_drop,
                                                              int* __restrict__ dw_counters, int nb_rows_, int cache_mode) {
  DROP_STEP(ddy); DROP_STEP(dout);
  __shared__ float red[4 * 256 * NV];  // [wave][col]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (dw_counters != nullptr && blockIdx.x == 0 && (int)threadIdx.x < (cols + 63) / 64) dw_counters[threadIdx.x] = 0;
  constexpr int nv = NV;
  float dwp[NV][4];
  float wv[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) dwp[i][e] = 0.f;
    if (i < nv) load4<float>(w + i * 256 + lane * 4, wv[i]);
  }
  const int row_end = min(rows, (int)(blockIdx.x + 1) * nb_rows_);
  for (int row = blockIdx.x * nb_rows_ + wave; row < row_end; row += 4) {
    const size_t base = (size_t)row * cols;
    const float rstd = rstd_in[row];
    float g[NV][4], xh[NV][4], rr[NV][4];
    float dot = 0.f;
    // the residual gradient is requested together with the other operands: one memory round trip per row, not two
    if (dres != nullptr) {
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (i < nv) {
          if (cache_mode & 4) load4_nt<TRI>(dres + base + i * 256 + lane * 4, rr[i]);
          else load4<TRI>(dres + base + i * 256 + lane * 4, rr[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (i < nv) {
        const int col = i * 256 + lane * 4;
        load4<TG>(dxn + base + col, g[i]);
        if (out_drop) mask4(dout, (base + col) >> 2, g[i]);     // (the site dropped its output: the stand-alone kernel only)
        if (cache_mode & 1) load4_nt<float>(x1 + base + col, xh[i]);
        else load4<float>(x1 + base + col, xh[i]);
        dot = norm_bwd_acc(g[i], xh[i], wv[i], rstd, dwp[i], dot);
      }
    }
    dot = norm_bwd_mean(wave_sum(dot), (float)cols);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (i < nv) {
        const int col = i * 256 + lane * 4;
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = norm_bwd_dx(g[i][e], xh[i][e], rstd, dot);
        if (dres != nullptr) add4(d, rr[i]);
        if (cache_mode & 2) store4_nt<TRO>(dx1 + base + col, d);
        else store4<TRO>(dx1 + base + col, d);
        if (dy != nullptr) {
          mask4(ddy, (base + col) >> 2, d);
          store4<bf16_t>(dy + base + col, d);
        }
      }
    }
  }
  // reduce dw partials across the 4 waves, then one atomic per column
  float* redf = &red[0];
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (i < nv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) redf[wave * cols + i * 256 + lane * 4 + e] = dwp[i][e];
    }
  __syncthreads();
  // per-workgroup partial -> workspace row (no atomics: 2048 workgroups hammering the same 512
  // addresses ran at the contended-atomic rate); dw_reduce_kernel sums the rows in a fixed order
  if (dw_part != nullptr)
    for (int c = threadIdx.x; c < cols; c += 256)
      dw_part[(size_t)blockIdx.x * cols + c] = redf[c] + redf[cols + c] + redf[2 * cols + c] + redf[3 * cols + c];
}

// dw[c] += sum over partial rows.  grid = (cols/64, DW_CHUNKS row chunks); a thread = (column, 1 of 4 row
// groups) streams its rows with independent loads, the workgroup combines through LDS and leaves its 64 sums in
// scratch[chunk]; the chunk workgroup that finishes last (agent-scope counter, zeroed by the norm-backward
// kernel before) adds the DW_CHUNKS partials in chunk order: no float atomics, bitwise reproducible.
__device__ __forceinline__ void dw_reduce_body(const float* __restrict__ part, float* __restrict__ dw, int n_part, int cols,
                                               float* __restrict__ scratch, int* __restrict__ counters) {
  // workgroup = 64 columns x one of DW_CHUNKS row chunks.  A thread = 4 columns (one 16-byte load per row) x 1 of 16
  // row groups, its rows requested eight at a time: the kernel is a handful of wide, independent loads per thread
  // instead of a long chain of 4-byte ones (550 -> 60 us for the 42 norm sites of a training step).
  __shared__ float red[16][64];
  __shared__ int last;
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c4 = blockIdx.x * 64 + q * 4;
  const int per = (n_part + gridDim.y - 1) / gridDim.y;
  const int r0 = blockIdx.y * per, r1 = min(n_part, r0 + per);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (c4 < cols) {
    int i = r0 + g;
    for (; i + 7 * 16 < r1; i += 8 * 16) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(part + (size_t)(i + u * 16) * cols + c4);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; i < r1; i += 16) acc += *(const f32x4*)(part + (size_t)i * cols + c4);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[g][q * 4 + e] = acc[e];
  __syncthreads();
  const int c = blockIdx.x * 64 + (int)threadIdx.x;
  if (threadIdx.x < 64 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
    __hip_atomic_store(&scratch[(size_t)blockIdx.y * cols + c], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // hand-off to the last-arriving chunk without __threadfence(): on gfx950 that is a write-back + invalidate of the
  // XCD's whole L2 per workgroup (5376 of them in the batched launch: 500-900 us for 168 MB).  Agent-scope relaxed
  // atomics (sc1: written through / read around the L2 per instruction), stores complete before the barrier.
  // This is NOT a release/acquire pair in the HIP memory model: it leans on gfx950 behaviour — an
  // acknowledged sc1 store (s_waitcnt vmcnt(0)) is visible to every later sc1 load of the device, and the inline-asm
  // wait is a compiler barrier — hence the architecture check below; profiles/tools/norm_dw_stress.py is the stress
  // test (900 iterations x 20 sites, alone and beside a second process: every result bit-identical).
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "dw_reduce_body's fence-free hand-off is validated on gfx950 only"
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(&counters[blockIdx.x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.y - 1;
  __syncthreads();
  if (!last) return;
  if (threadIdx.x < 64 && c < cols) {
    float a = dw[c];
    for (int k = 0; k < (int)gridDim.y; ++k)
      a += __hip_atomic_load(&scratch[(size_t)k * cols + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    dw[c] = a;
  }
  if (threadIdx.x == 0) __hip_atomic_store(&counters[blockIdx.x], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ __launch_bounds__(256) void dw_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                        int n_part, int cols, float* __restrict__ scratch,
                                                        int* __restrict__ counters) {
  dw_reduce_body(part, dw, n_part, cols, scratch, counters);
}
// the same reduction for several norm sites in one launch (blockIdx.z = site): the engine leaves each site's partial
// rows in a workspace of its own during backward and sums them all when a gradient bucket is about to be sent
__global__ __launch_bounds__(256) void dw_reduce_sites_kernel(const unsigned long long* __restrict__ ws, const unsigned long long* __restrict__ dws,
                                                              const int* __restrict__ n_parts, int cols) {
  const int site = blockIdx.z, n_part = n_parts[site];
  float* part = (float*)ws[site];
  float* scratch = part + (size_t)n_part * cols;
  dw_reduce_body(part, (float*)dws[site], n_part, cols, scratch, (int*)(scratch + (size_t)DW_CHUNKS * cols));
}

extern "C" int mrmt3_add_rmsnorm_bwd_partial_rows(int rows) { return ceil_div(rows, nb_rows(rows)); }

extern "C" int mrmt3_norm_dw_reduce(const void* workspaces, const void* dws, const int* partial_rows, int n_sites, int cols,
                                    void* stream) {
  MR_CHECK_ARG(workspaces && dws && partial_rows, "norm_dw_reduce: null pointer");
  MR_CHECK_ARG(n_sites > 0 && n_sites <= 65535 && cols > 0, "norm_dw_reduce: bad sizes");
  hipLaunchKernelGGL(dw_reduce_sites_kernel, dim3((unsigned)ceil_div(cols, 64), DW_CHUNKS, (unsigned)n_sites), dim3(256), 0,
                     (hipStream_t)stream, (const unsigned long long*)workspaces, (const unsigned long long*)dws, partial_rows, cols);
  MR_CHECK_LAUNCH("norm_dw_reduce");
  return MRMT3_OK;
}

extern "C" size_t mrmt3_add_rmsnorm_bwd_workspace_bytes(int rows, int cols) {
  // per-workgroup partial rows | DW_CHUNKS chunk sums | one arrival counter per 64 columns
  return ((size_t)ceil_div(rows, nb_rows(rows)) + DW_CHUNKS) * cols * sizeof(float) + (size_t)ceil_div(cols, 64) * sizeof(int);
}

extern "C" int mrmt3_add_rmsnorm_bwd(const void* dxn, int dxn_dtype, const void* dres, int dres_dtype, const float* x1,
                                     const float* rstd, const float* w, void* dx1, int dx1_dtype, void* dy_bf16,
                                     float* dw, int rows, int cols,
                                     float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_y, uint32_t stream_out,
                                     int out_drop, void* workspace, size_t workspace_bytes, void* stream) {
  MR_CHECK_ARG(dw == nullptr || workspace, "add_rmsnorm_bwd: dw needs a workspace");
  MR_CHECK_ARG(workspace == nullptr || workspace_bytes >= mrmt3_add_rmsnorm_bwd_workspace_bytes(rows, cols),
               "add_rmsnorm_bwd: workspace too small");
  // workspace without dw: the partial rows are left for mrmt3_norm_dw_reduce (deferred, batched over sites)
  float* dw_part = (float*)workspace;
  const int nbr = nb_rows(rows);
  float* dw_scratch = workspace ? dw_part + (size_t)ceil_div(rows, nbr) * cols : nullptr;
  int* dw_counters = workspace ? (int*)(dw_scratch + (size_t)DW_CHUNKS * cols) : nullptr;
  MR_CHECK_ARG(dxn && x1 && rstd && w && dx1, "add_rmsnorm_bwd: null pointer");
  MR_CHECK_ARG(rows > 0 && (cols == 256 || cols == 512 || cols == 1024 || cols == 2048),
               "add_rmsnorm_bwd: cols must be 256, 512, 1024 or 2048");
  MR_CHECK_DTYPE("add_rmsnorm_bwd", dxn_dtype);
  MR_CHECK_DTYPE("add_rmsnorm_bwd", dres_dtype);
  MR_CHECK_DTYPE("add_rmsnorm_bwd", dx1_dtype);
  // bf16 residual-gradient stream (the engine's bf16 path): model width 512 only.  A null dres takes the float kernels.
  const int tri_dtype = dres ? dres_dtype : MRMT3_F32;
  MR_CHECK_ARG((tri_dtype == MRMT3_F32 && dx1_dtype == MRMT3_F32) || cols == 512,
               "add_rmsnorm_bwd: a bf16 residual gradient needs cols == 512");
  DropCfg dy = make_drop(p_drop, seed, stream_y, step_dev), dn = make_drop(p_drop, seed, stream_out, step_dev);
  // bit 0: streaming load of x1 (the saved residual stream: read once), bit 1: streaming store of dx1 (the residual
  // gradient: its reader is the next norm backward), bit 2: streaming load of dres (MRMT3_NORMB_NT).  Measured: none of
  // them moves the 64-segment step (25.61-25.80 ms against 25.61-25.68, two alternations) — off.
  const int cache_mode = MR_KNOB("MRMT3_NORMB_NT", 0);
  mr_dtype(dxn_dtype, [&](auto tg) {
    mr_dtype(tri_dtype, [&](auto tri) {
      mr_dtype(dx1_dtype, [&](auto tro) {
        mr_const<1, 2, 4, 8>(cols / 256, [&](auto nv) {
          using TG = typename decltype(tg)::type;
          using TRI = typename decltype(tri)::type;
          using TRO = typename decltype(tro)::type;
          constexpr int NV = decltype(nv)::value;
          // the bf16 residual kernels exist at NV = 2 alone (the argument check above)
          if constexpr (NV == 2 || (sizeof(TRI) == 4 && sizeof(TRO) == 4))
            hipLaunchKernelGGL((add_rmsnorm_bwd_kernel<NV, TG, TRI, TRO>), dim3((unsigned)ceil_div(rows, nbr)), dim3(256), 0,
                               (hipStream_t)stream, (const TG*)dxn, (const TRI*)dres, x1, rstd, w, (TRO*)dx1,
                               (bf16_t*)dy_bf16, dw_part, rows, cols, dy, dn, out_drop, dw_counters, nbr, cache_mode);
        });
      });
    });
  });
  MR_CHECK_LAUNCH("add_rmsnorm_bwd");
  if (dw) {
    hipLaunchKernelGGL(dw_reduce_kernel, dim3((unsigned)ceil_div(cols, 64), DW_CHUNKS), dim3(256), 0, (hipStream_t)stream,
                       (const float*)dw_part, dw, ceil_div(rows, nbr), cols, dw_scratch, dw_counters);
    MR_CHECK_LAUNCH("add_rmsnorm_bwd dw reduce");
  }
  return MRMT3_OK;
}

// ------------------------------------------------------------------------------------------------
// gated GELU (HF T5DenseGatedGeluDense + NewGELUActivation)
// ------------------------------------------------------------------------------------------------
// Both kernels move 8 elements (two dropout quads) per thread and iteration: 16-byte accesses for bf16.
template <typename T>
__global__ void geglu_fwd_kernel(const T* __restrict__ h, int ldh, T* __restrict__ g, int ldg, int rows, int dff, DropCfg d) {
  DROP_STEP(d);
  const size_t n8 = (size_t)rows * dff / 8;
  const int dff8 = dff / 8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / dff8;
    const int col = (int)(i % dff8) * 8;
    float a[8], b[8], o[8];
    load4<T>(h + row * ldh + col, a);
    load4<T>(h + row * ldh + col + 4, a + 4);
    load4<T>(h + row * ldh + dff + col, b);
    load4<T>(h + row * ldh + dff + col + 4, b + 4);
    geglu_fwd8(d, 2 * i, a, b, o);                 // (the mask index is the element's index in a dense [rows][dff])
    store4<T>(g + row * ldg + col, o);
    store4<T>(g + row * ldg + col + 4, o + 4);
  }
}

template <typename T>
__global__ void geglu_bwd_kernel(const T* __restrict__ h, const T* __restrict__ dg, T* __restrict__ dh,
                                 int rows, int dff, DropCfg d, int cache_mode) {
  DROP_STEP(d);
  const size_t n8 = (size_t)rows * dff / 8;
  const int dff8 = dff / 8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / dff8;
    const int col = (int)(i % dff8) * 8;
    float a[8], b[8], go[8], da[8], db[8];
    if (cache_mode & 1) {                       // h: the saved projection, read once
      load4_nt<T>(h + row * 2 * dff + col, a);
      load4_nt<T>(h + row * 2 * dff + col + 4, a + 4);
      load4_nt<T>(h + row * 2 * dff + dff + col, b);
      load4_nt<T>(h + row * 2 * dff + dff + col + 4, b + 4);
    } else {
      load4<T>(h + row * 2 * dff + col, a);
      load4<T>(h + row * 2 * dff + col + 4, a + 4);
      load4<T>(h + row * 2 * dff + dff + col, b);
      load4<T>(h + row * 2 * dff + dff + col + 4, b + 4);
    }
    load4<T>(dg + row * dff + col, go);
    load4<T>(dg + row * dff + col + 4, go + 4);
    geglu_bwd8(d, 2 * i, a, b, go, da, db);
    store4<T>(dh + row * 2 * dff + col, da);
    store4<T>(dh + row * 2 * dff + col + 4, da + 4);
    store4<T>(dh + row * 2 * dff + dff + col, db);
    store4<T>(dh + row * 2 * dff + dff + col + 4, db + 4);
  }
}

// h [rows][ldh] and g [rows][ldg] as views of wider buffers (ldh, ldg in elements): the second half of the unfused
// mrmt3_gemm_nt_geglu (gemm8.hip).  Same arithmetic and the same mask as the dense form: the mask follows (row, feature).
int mrmt3_geglu_fwd_ld(const void* h, int ldh, void* g, int ldg, int rows, int dff, int dtype, float p_drop, uint64_t seed,
                       const int32_t* step_dev, uint32_t stream_id, void* stream) {
  MR_CHECK_ARG(h && g && rows > 0 && dff % 8 == 0, "geglu_fwd: bad args");
  MR_CHECK_DTYPE("geglu_fwd", dtype);
  MR_CHECK_ARG(ldh >= 2 * dff && ldg >= dff && ldh % 8 == 0 && ldg % 8 == 0, "geglu_fwd: ldh >= 2 dff, ldg >= dff, both multiples of 8");
  DropCfg d = make_drop(p_drop, seed, stream_id, step_dev);
  const int blocks = ew_blocks((size_t)rows * dff / 8);
  mr_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(geglu_fwd_kernel<T>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)h, ldh, (T*)g, ldg, rows, dff, d);
  });
  MR_CHECK_LAUNCH("geglu_fwd");
  return MRMT3_OK;
}

extern "C" int mrmt3_geglu_fwd(const void* h, void* g, int rows, int dff, int dtype, float p_drop, uint64_t seed, const int32_t* step_dev,
                               uint32_t stream_id, void* stream) {
  return mrmt3_geglu_fwd_ld(h, 2 * dff, g, dff, rows, dff, dtype, p_drop, seed, step_dev, stream_id, stream);
}

extern "C" int mrmt3_geglu_bwd(const void* h, const void* dg, void* dh, int rows, int dff, int dtype, float p_drop,
                               uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream) {
  MR_CHECK_ARG(h && dg && dh && rows > 0 && dff % 8 == 0, "geglu_bwd: bad args");
  MR_CHECK_DTYPE("geglu_bwd", dtype);
  DropCfg d = make_drop(p_drop, seed, stream_id, step_dev);
  const int cm = MR_KNOB("MRMT3_GEGLUB_NT", 0);      // bit 0: streaming load of h (measured: no change; off)
  mr_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(geglu_bwd_kernel<T>, dim3(ew_blocks((size_t)rows * dff / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)h, (const T*)dg, (T*)dh, rows, dff, d, cm);
  });
  MR_CHECK_LAUNCH("geglu_bwd");
  return MRMT3_OK;
}

