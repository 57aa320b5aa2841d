// Token embedding: the gather (+ _shift_right) + sinusoid add + dropout forward, its sorted, atomic-free gradient (eb_*),
// the sinusoid add alone (addpos) and the dropout mask applied to a gradient on its way to another dtype (dropmask_cast).
// (The packed-row gather embed_fwd_packed lives in pack.hip.)
#include "common.h"
#include "rowmath.h"

// no implicit FMA formation in this file: the run sums of the embedding gradient (eb_sum_kernel: acc += dx * mask, a product
// rounded before it is added) have their bits pinned under this setting
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// embedding gather (+ _shift_right) + sinusoid add + dropout; scatter-add backward
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t token_at(const int64_t* ids, int row, int seq_len, int shift, int start_id,
                                            int pad_id, int vocab) {
  int64_t id;
  if (shift) {
    const int t = row % seq_len;
    id = (t == 0) ? start_id : ids[row - 1];
    if (id == -100) id = pad_id;
  } else {
    id = ids[row];
  }
  if (id < 0) id = 0;
  if (id >= vocab) id = vocab - 1;
  return id;
}

__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table,
                                                        const float* __restrict__ pos, float* __restrict__ x, int rows,
                                                        int seq_len, int d, int vocab, int shift, int start_id,
                                                        int pad_id, int pos_offset, DropCfg dc) {
  DROP_STEP(dc);
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t id = token_at(ids, row, seq_len, shift, start_id, pad_id, vocab);
  const float* trow = table + (size_t)id * d;
  const float* prow = pos ? pos + (size_t)((row % seq_len) + pos_offset) * d : nullptr;
  const size_t base = (size_t)row * d;
  for (int col = lane * 4; col < d; col += 256) {
    float a[4], p[4];
    load4<float>(trow + col, a);
    if (prow) {
      load4<float>(prow + col, p);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += p[e];
    }
    if (dc.thresh) {
      float m[4];
      drop_mask4(dc, (base + col) >> 2, m);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] *= m[e];
    }
    store4<float>(x + base + col, a);
  }
}

// ---- embedding gradient: dtable[id] += dropmask(dx[row]) without atomics -------------------------------------
// Token ids of a transcription target are heavily skewed (a handful of velocity / program ids, and every padded
// position maps to id 0), so a scatter-add with f32 atomics serialises on a few table rows and is order-dependent.
// Instead the rows are ranked by id with a counting sort (per-workgroup histograms -> column scan -> stable
// scatter), chunks of EB_CHUNK sorted rows are summed run by run, and the runs that cross a chunk boundary are
// combined per id in chunk order: every table row has one writer and the result is bitwise reproducible.
#define EB_ROWS 256     // rows ranked per workgroup
#define EB_CHUNK 32     // sorted rows summed per workgroup
struct EbPlan { int n_wg, n_chunk; size_t off_hist, off_base, off_order, off_tok, off_part, total; };
static EbPlan eb_plan(int rows, int vocab, int d) {
  EbPlan p;
  p.n_wg = ceil_div(rows, EB_ROWS);
  p.n_chunk = ceil_div(rows, EB_CHUNK);
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  p.off_hist = take((size_t)p.n_wg * vocab * 4);          // [n_wg][vocab] counts, then exclusive offsets inside an id
  p.off_base = take((size_t)(vocab + 1) * 4);             // first sorted position of every id
  p.off_order = take((size_t)rows * 4);                   // sorted position -> row
  p.off_tok = take((size_t)rows * 4);                     // row -> id
  p.off_part = take((size_t)p.n_chunk * 2 * d * 4);       // [chunk][first|last run][d] partial sums
  p.total = o;
  return p;
}

__global__ __launch_bounds__(EB_ROWS) void eb_hist_kernel(const int64_t* __restrict__ ids, int* __restrict__ tok,
                                                           int* __restrict__ hist, int rows, int seq_len, int vocab,
                                                           int shift, int start_id, int pad_id) {
  extern __shared__ int h[];
  for (int v = threadIdx.x; v < vocab; v += EB_ROWS) h[v] = 0;
  __syncthreads();
  const int row = blockIdx.x * EB_ROWS + threadIdx.x;
  if (row < rows) {
    const int id = (int)token_at(ids, row, seq_len, shift, start_id, pad_id, vocab);
    tok[row] = id;
    atomicAdd(&h[id], 1);                                   // LDS counter: only the count matters here
  }
  __syncthreads();
  for (int v = threadIdx.x; v < vocab; v += EB_ROWS) hist[(size_t)blockIdx.x * vocab + v] = h[v];
}

// per id: exclusive scan of the workgroup counts (in place) and the id's total.  A workgroup owns 32 ids; the
// n_wg counts of an id are cut into 8 segments scanned by 8 threads (sum, scan of the 8 sums in LDS, rescan).
__global__ __launch_bounds__(256) void eb_scan_wg_kernel(int* __restrict__ hist, int* __restrict__ base, int n_wg, int vocab) {
  __shared__ int seg_sum[8][32];
  const int vi = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int v = blockIdx.x * 32 + vi;
  const int per = ceil_div(n_wg, 8), g0 = sg * per, g1 = min(n_wg, g0 + per);
  int s = 0;
  if (v < vocab)
    for (int g = g0; g < g1; ++g) s += hist[(size_t)g * vocab + v];
  seg_sum[sg][vi] = s;
  __syncthreads();
  int run = 0;
  for (int k = 0; k < sg; ++k) run += seg_sum[k][vi];
  if (v >= vocab) return;
  for (int g = g0; g < g1; ++g) {
    const int c = hist[(size_t)g * vocab + v];
    hist[(size_t)g * vocab + v] = run;
    run += c;
  }
  if (sg == 7) base[v] = run;                               // totals for now
}
// exclusive scan of the totals over the ids (one workgroup; vocab is a few thousand at most)
__global__ __launch_bounds__(1024) void eb_scan_ids_kernel(int* __restrict__ base, int vocab) {
  __shared__ int part[1024];
  const int per = ceil_div(vocab, 1024);
  const int lo = threadIdx.x * per, hi = min(vocab, lo + per);
  int s = 0;
  for (int v = lo; v < hi; ++v) s += base[v];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < 1024; ++i) { const int c = part[i]; part[i] = run; run += c; }
    base[vocab] = run;
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int v = lo; v < hi; ++v) { const int c = base[v]; base[v] = run; run += c; }
}

__global__ __launch_bounds__(EB_ROWS) void eb_scatter_kernel(const int* __restrict__ tok, const int* __restrict__ hist,
                                                              const int* __restrict__ base, int* __restrict__ order,
                                                              int rows, int vocab) {
  __shared__ int t[EB_ROWS];
  const int row = blockIdx.x * EB_ROWS + threadIdx.x;
  const int mine = row < rows ? tok[row] : -1;
  t[threadIdx.x] = mine;
  __syncthreads();
  if (row >= rows) return;
  int rank = 0;                                             // earlier rows of this workgroup with the same id: stable
  for (int j = 0; j < (int)threadIdx.x; ++j) rank += (t[j] == mine);
  order[base[mine] + hist[(size_t)blockIdx.x * vocab + mine] + rank] = row;
}

// one workgroup sums EB_CHUNK consecutive sorted rows run by run.  A run that starts and ends inside the chunk has
// all of its id's rows here: it is added to the table directly.  The chunk's first and last run may continue in
// the neighbouring chunks: their sums go to part[chunk][0 / 1] and eb_combine_kernel adds them per id.
__global__ __launch_bounds__(256) void eb_sum_kernel(const int* __restrict__ order, const int* __restrict__ tok,
                                                      const int* __restrict__ base, const float* __restrict__ dx,
                                                      float* __restrict__ dtable, float* __restrict__ part, int rows,
                                                      int d, DropCfg dc) {
  DROP_STEP(dc);
  __shared__ int srow[EB_CHUNK], sid[EB_CHUNK];
  const int p0 = blockIdx.x * EB_CHUNK, n = min(EB_CHUNK, rows - p0);
  if (threadIdx.x < n) {
    const int r = order[p0 + threadIdx.x];
    srow[threadIdx.x] = r;
    sid[threadIdx.x] = tok[r];
  }
  __syncthreads();
  for (int col = threadIdx.x * 4; col < d; col += 1024) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int run_start = 0;
    for (int i = 0; i < n; ++i) {
      float a[4];
      const size_t at = (size_t)srow[i] * d + col;
      load4<float>(dx + at, a);
      if (dc.thresh) {
        float m[4];
        drop_mask4(dc, at >> 2, m);
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] *= m[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += a[e];
      if (i + 1 == n || sid[i + 1] != sid[i]) {             // the run [run_start, i] of id sid[i] ends here
        const int id = sid[i];
        const bool whole = base[id] >= p0 + run_start && base[id + 1] <= p0 + i + 1;   // all rows of the id are in it
        float* dst = whole ? dtable + (size_t)id * d + col
                           : part + ((size_t)blockIdx.x * 2 + (run_start == 0 ? 0 : 1)) * d + col;
        if (whole) {
          float o[4];
          load4<float>(dst, o);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] += o[e];
        }
        store4<float>(dst, acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = 0.f;
        run_start = i + 1;
      }
    }
  }
}

// ids whose rows span several chunks: add the chunks' partial sums in chunk order
__global__ __launch_bounds__(128) void eb_combine_kernel(const int* __restrict__ base, const float* __restrict__ part,
                                                          float* __restrict__ dtable, int d) {
  const int id = blockIdx.x;
  const int lo = base[id], hi = base[id + 1];
  if (hi <= lo) return;
  const int c0 = lo / EB_CHUNK, c1 = (hi - 1) / EB_CHUNK;
  if (c0 == c1 && lo >= c0 * EB_CHUNK && hi <= (c0 + 1) * EB_CHUNK) return;      // a whole run: already in the table
  for (int col = threadIdx.x * 4; col < d; col += 512) {
    float acc[4];
    load4<float>(dtable + (size_t)id * d + col, acc);
    for (int c = c0; c <= c1; ++c) {
      // in chunk c the id's run is the first one unless it starts inside the chunk
      const int slot = (lo > c * EB_CHUNK) ? 1 : 0;
      float a[4];
      load4<float>(part + ((size_t)c * 2 + slot) * d + col, a);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += a[e];
    }
    store4<float>(dtable + (size_t)id * d + col, acc);
  }
}

extern "C" int mrmt3_embed_fwd(const int64_t* ids, const float* table, const float* pos, float* x, int rows,
                               int seq_len, int d, int vocab, int shift, int start_id, int pad_id, int pos_offset,
                               float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id, void* stream) {
  MR_CHECK_ARG(ids && table && x && rows > 0 && seq_len > 0 && d % 4 == 0, "embed_fwd: bad args");
  hipLaunchKernelGGL(embed_fwd_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, ids,
                     table, pos, x, rows, seq_len, d, vocab, shift, start_id, pad_id, pos_offset,
                     make_drop(p_drop, seed, stream_id, step_dev));
  MR_CHECK_LAUNCH("embed_fwd");
  return MRMT3_OK;
}

extern "C" size_t mrmt3_embed_bwd_workspace_bytes(int rows, int vocab, int d) { return eb_plan(rows, vocab, d).total; }

extern "C" int mrmt3_embed_bwd(const int64_t* ids, const float* dx, float* dtable, int rows, int seq_len, int d,
                               int vocab, int shift, int start_id, int pad_id, float p_drop, uint64_t seed, const int32_t* step_dev,
                               uint32_t stream_id, void* workspace, size_t workspace_bytes, void* stream) {
  MR_CHECK_ARG(ids && dx && dtable && workspace && rows > 0 && seq_len > 0 && d % 4 == 0 && vocab > 0,
               "embed_bwd: bad args");
  MR_CHECK_ARG(vocab * (int)sizeof(int) <= 64 * 1024, "embed_bwd: vocabulary too large for the LDS histogram");
  const EbPlan P = eb_plan(rows, vocab, d);
  MR_CHECK_ARG(workspace_bytes >= P.total, "embed_bwd: workspace too small");
  unsigned char* ws = (unsigned char*)workspace;
  int* hist = (int*)(ws + P.off_hist);
  int* base = (int*)(ws + P.off_base);
  int* order = (int*)(ws + P.off_order);
  int* tok = (int*)(ws + P.off_tok);
  float* part = (float*)(ws + P.off_part);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(eb_hist_kernel, dim3(P.n_wg), dim3(EB_ROWS), vocab * sizeof(int), s, ids, tok, hist, rows, seq_len,
                     vocab, shift, start_id, pad_id);
  hipLaunchKernelGGL(eb_scan_wg_kernel, dim3(ceil_div(vocab, 32)), dim3(256), 0, s, hist, base, P.n_wg, vocab);
  hipLaunchKernelGGL(eb_scan_ids_kernel, dim3(1), dim3(1024), 0, s, base, vocab);
  hipLaunchKernelGGL(eb_scatter_kernel, dim3(P.n_wg), dim3(EB_ROWS), 0, s, tok, hist, base, order, rows, vocab);
  hipLaunchKernelGGL(eb_sum_kernel, dim3(P.n_chunk), dim3(256), 0, s, order, tok, base, dx, dtable, part, rows, d,
                     make_drop(p_drop, seed, stream_id, step_dev));
  hipLaunchKernelGGL(eb_combine_kernel, dim3(vocab), dim3(128), 0, s, base, part, dtable, d);
  MR_CHECK_LAUNCH("embed_bwd");
  return MRMT3_OK;
}

template <typename T>
__global__ void addpos_fwd_kernel(const T* __restrict__ src, const float* __restrict__ pos, float* __restrict__ x,
                                  size_t n4, int seq_len, int d, int pos_offset, DropCfg dc) {
  DROP_STEP(dc);
  const int d4 = d / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / d4;
    const int col = (int)(i % d4) * 4;
    float a[4], p[4];
    load4<T>(src + i * 4, a);
    load4<float>(pos + (size_t)((row % seq_len) + pos_offset) * d + col, p);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += p[e];
    if (dc.thresh) {
      float m[4];
      drop_mask4(dc, i, m);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] *= m[e];
    }
    store4<float>(x + i * 4, a);
  }
}

extern "C" int mrmt3_addpos_fwd(const void* src, int src_dtype, const float* pos, float* x, int rows, int seq_len,
                                int d, int pos_offset, float p_drop, uint64_t seed, const int32_t* step_dev, uint32_t stream_id,
                                void* stream) {
  MR_CHECK_ARG(src && pos && x && rows > 0 && seq_len > 0 && d % 4 == 0, "addpos_fwd: bad args");
  MR_CHECK_DTYPE("addpos_fwd", src_dtype);
  const size_t n4 = (size_t)rows * d / 4;
  DropCfg dc = make_drop(p_drop, seed, stream_id, step_dev);
  mr_dtype(src_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(addpos_fwd_kernel<T>, dim3(ew_blocks(n4)), dim3(256), 0, (hipStream_t)stream, (const T*)src, pos, x,
                       n4, seq_len, d, pos_offset, dc);
  });
  MR_CHECK_LAUNCH("addpos_fwd");
  return MRMT3_OK;
}

template <typename TO>
__global__ void dropmask_cast_kernel(const float* __restrict__ dx, TO* __restrict__ out, size_t n4, DropCfg dc) {
  DROP_STEP(dc);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float a[4];
    load4<float>(dx + i * 4, a);
    if (dc.thresh) {
      float m[4];
      drop_mask4(dc, i, m);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] *= m[e];
    }
    store4<TO>(out + i * 4, a);
  }
}

extern "C" int mrmt3_dropmask_cast(const float* dx, void* out, int out_dtype, size_t n, float p_drop, uint64_t seed,
                                   const int32_t* step_dev, uint32_t stream_id, void* stream) {
  MR_CHECK_ARG(dx && out && n % 4 == 0, "dropmask_cast: bad args");
  MR_CHECK_DTYPE("dropmask_cast", out_dtype);
  mr_dtype(out_dtype, [&](auto t) {
    using TO = typename decltype(t)::type;
    hipLaunchKernelGGL(dropmask_cast_kernel<TO>, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, dx, (TO*)out,
                       n / 4, make_drop(p_drop, seed, stream_id, step_dev));
  });
  MR_CHECK_LAUNCH("dropmask_cast");
  return MRMT3_OK;
}

