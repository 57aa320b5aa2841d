// Cast and transpose helpers of the weight shadows: the bf16 copies of the f32 master weights and their pre-transposed
// dgrad copies (one matrix, or every weight of the model in one batched launch).
#include "common.h"
#include "rowmath.h"

// no implicit FMA formation in this file, as in the other four row sources: these kernels only convert (f2bf / bf2f) and
// move, so no bits depend on the setting today; arithmetic added to one of the copies later starts out pinned
#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// cast / transpose helpers (bf16 shadow weights and their pre-transposed dgrad copies)
// ------------------------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ void cast_kernel(const TI* __restrict__ in, TO* __restrict__ out, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float a[4];
    load4<TI>(in + i * 4, a);
    store4<TO>(out + i * 4, a);
  }
}

extern "C" int mrmt3_cast(const void* in, int in_dtype, void* out, int out_dtype, size_t n, void* stream) {
  MR_CHECK_ARG(in && out && n % 4 == 0, "cast: bad args");
  MR_CHECK_DTYPE("cast", in_dtype);
  MR_CHECK_DTYPE("cast", out_dtype);
  mr_dtype(in_dtype, [&](auto ti) {
    mr_dtype(out_dtype, [&](auto to) {
      using TI = typename decltype(ti)::type;
      using TO = typename decltype(to)::type;
      hipLaunchKernelGGL((cast_kernel<TI, TO>), dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, (const TI*)in,
                         (TO*)out, n / 4);
    });
  });
  MR_CHECK_LAUNCH("cast");
  return MRMT3_OK;
}

template <typename TI, typename TO>
__global__ void transpose_kernel(const TI* __restrict__ in, TO* __restrict__ out, int rows, int cols) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int r = by + j, c = bx + tx;
    float v = 0.f;
    if (r < rows && c < cols) {
      if constexpr (sizeof(TI) == 2) v = bf2f(in[(size_t)r * cols + c]);
      else v = in[(size_t)r * cols + c];
    }
    tile[j][tx] = v;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = bx + j, r = by + tx;  // out[c][r]
    if (r < rows && c < cols) {
      const float v = tile[tx][j];
      if constexpr (sizeof(TO) == 2) out[(size_t)c * rows + r] = f2bf(v);
      else out[(size_t)c * rows + r] = v;
    }
  }
}

// batched bf16 transpose of many small matrices described by a device table of
// {src_off, dst_off, rows, cols} (element offsets) — one launch refreshes every pre-transposed weight.
// 64x64 tiles; both sides move element PAIRS (4 bytes per lane, 128 contiguous bytes per 32 lanes) when the
// matrix dimensions and offsets are even, single elements otherwise.
#define TRB 64
struct TrDesc { long long src, dst; int rows, cols; };
__global__ __launch_bounds__(256) void transpose_batched_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                                const TrDesc* __restrict__ tab,
                                                                const int* __restrict__ tile_start, int n_mats) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[TRB][TRB + 2];
  // find the matrix this block belongs to (tile_start is a prefix sum of 64x64 tile counts)
  int m = 0;
  while (m + 1 < n_mats && (int)blockIdx.x >= tile_start[m + 1]) ++m;
  const TrDesc d = tab[m];
  const int local = blockIdx.x - tile_start[m];
  const int tiles_x = (d.cols + TRB - 1) / TRB;
  const int bx = (local % tiles_x) * TRB, by = (local / tiles_x) * TRB;
  // fast path (every weight of the model): a tile inside a matrix whose dimensions and offsets are multiples of 8 moves
  // 16 bytes per lane on both sides — a lane loads 8 consecutive columns of a row, stores them as four dwords (row stride
  // 66 elements = 33 dwords: the transposed 2-byte reads of a wave then touch 32 different banks), reads 8 consecutive
  // ROWS of one column back and stores them as 16 bytes of the transposed row.
  if ((((d.rows | d.cols) & 7) == 0) && (((d.src | d.dst) & 7) == 0) && bx + TRB <= d.cols && by + TRB <= d.rows) {
    const int r = threadIdx.x >> 3, c8 = threadIdx.x & 7;
    unsigned* t32 = (unsigned*)&tile[0][0];                     // row stride 33 dwords
#pragma unroll
    for (int hlf = 0; hlf < 2; ++hlf) {
      const int rr = r + 32 * hlf;
      const u32x4 v = *(const u32x4*)(src + d.src + (size_t)(by + rr) * d.cols + bx + c8 * 8);
      unsigned* q = t32 + rr * 33 + c8 * 4;
      q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int hlf = 0; hlf < 2; ++hlf) {
      const int oc = r + 32 * hlf;                              // output row = source column
      unsigned w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        w[k] = (unsigned)tile[c8 * 8 + 2 * k][oc] | ((unsigned)tile[c8 * 8 + 2 * k + 1][oc] << 16);
      *(u32x4*)(dst + d.dst + (size_t)(bx + oc) * d.rows + by + c8 * 8) = u32x4{w[0], w[1], w[2], w[3]};
    }
    return;
  }
  const int tp = threadIdx.x & 31, ty = threadIdx.x >> 5;      // pair index, 8 row groups
  const bool even = ((d.rows | d.cols) & 1) == 0 && ((d.src | d.dst) & 1) == 0;
  for (int j = ty; j < TRB; j += 8) {
    const int r = by + j, c = bx + 2 * tp;
    bf16_t v0 = 0, v1 = 0;
    if (r < d.rows) {
      const bf16_t* p = src + d.src + (size_t)r * d.cols + c;
      if (even && c + 1 < d.cols) {
        const unsigned u = *(const unsigned*)p;
        v0 = (bf16_t)(u & 0xFFFFu);
        v1 = (bf16_t)(u >> 16);
      } else {
        if (c < d.cols) v0 = p[0];
        if (c + 1 < d.cols) v1 = p[1];
      }
    }
    tile[j][2 * tp] = v0;
    tile[j][2 * tp + 1] = v1;
  }
  __syncthreads();
  for (int j = ty; j < TRB; j += 8) {
    const int c = bx + j, r = by + 2 * tp;                    // output row c holds source rows r, r+1 side by side
    if (c >= d.cols) continue;
    bf16_t* q = dst + d.dst + (size_t)c * d.rows + r;
    const bf16_t v0 = tile[2 * tp][j], v1 = tile[2 * tp + 1][j];
    if (even && r + 1 < d.rows) *(unsigned*)q = (unsigned)v0 | ((unsigned)v1 << 16);
    else {
      if (r < d.rows) q[0] = v0;
      if (r + 1 < d.rows) q[1] = v1;
    }
  }
}

extern "C" int mrmt3_transpose_batched(const void* src_bf16, void* dst_bf16, const void* desc_table,
                                       const int* tile_start, int n_mats, int total_tiles, void* stream) {
  MR_CHECK_ARG(src_bf16 && dst_bf16 && desc_table && tile_start && n_mats > 0 && total_tiles > 0, "transpose_batched: bad args");
  hipLaunchKernelGGL(transpose_batched_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)src_bf16, (bf16_t*)dst_bf16, (const TrDesc*)desc_table, tile_start, n_mats);
  MR_CHECK_LAUNCH("transpose_batched");
  return MRMT3_OK;
}

extern "C" int mrmt3_transpose(const void* in, int in_dtype, void* out, int out_dtype, int rows, int cols,
                               void* stream) {
  MR_CHECK_ARG(in && out && rows > 0 && cols > 0, "transpose: bad args");
  MR_CHECK_DTYPE("transpose", in_dtype);
  MR_CHECK_DTYPE("transpose", out_dtype);
  dim3 grid((unsigned)ceil_div(cols, 32), (unsigned)ceil_div(rows, 32)), block(256);
  mr_dtype(in_dtype, [&](auto ti) {
    mr_dtype(out_dtype, [&](auto to) {
      using TI = typename decltype(ti)::type;
      using TO = typename decltype(to)::type;
      hipLaunchKernelGGL((transpose_kernel<TI, TO>), grid, block, 0, (hipStream_t)stream, (const TI*)in, (TO*)out, rows, cols);
    });
  });
  MR_CHECK_LAUNCH("transpose");
  return MRMT3_OK;
}
