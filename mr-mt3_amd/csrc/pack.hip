// Packed decoder rows: the plan that drops every position after a row's last scored label, and the embedding of the packed rows.
//
// A target row is padded to L with -100 (the reference's collate, dataset/dataset_2_random.py:292-306) and the loss ignores
// those positions.  Under the causal decoder a position after the row's last scored label cannot reach a scored one and its
// own gradient is zero, so the decoder only needs each row's prefix len_b = 1 + (last t with labels[b, t] != -100), 0 for a
// row with none.  The rows are laid end to end: row b owns packed rows [row_off[b], row_off[b+1]), T = row_off[B] rows in
// all, padded to a capacity Tcap that the host picks from the lengths (a few signatures per batch shape, see mrmt3/packing.py).
// Packed rows [T, Tcap) are the tail: decoder input pad_id at position 0, target -100.
//
// mrmt3_pack_plan is one call of three small launches (row lengths; offsets + attention tile list in one workgroup; the
// per-token arrays), all reading the dense labels on the device, so a captured step replays it for any batch of the same Tcap.
#include "common.h"

#include "attn_common.h"

namespace {

// len[b] = 1 + last t with labels[b, t] != -100, else 0
__global__ __launch_bounds__(256) void pack_len_kernel(const int64_t* __restrict__ labels, int L, int* __restrict__ len) {
  __shared__ int red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t* row = labels + (size_t)b * L;
  int last = 0;
  for (int t = tid; t < L; t += 256)
    if (row[t] != -100) last = t + 1;
  last = (int)wave_max((float)last);       // (exact: lengths are far below 2^24)
  if ((tid & 63) == 0) red[tid >> 6] = last;
  __syncthreads();
  if (tid == 0) len[b] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// one workgroup: row_off (clamped to Tcap, so every later index stays inside the buffers even when T > Tcap: that case also
// sets *err), then the tile list of the varlen attention kernels — for t from the largest tile index down to 0, the rows that
// have a tile t, in row order.  Thread j builds the group of tile index j (at most 1024 tiles of 64 rows per row).
__global__ __launch_bounds__(1024) void pack_index_kernel(const int* __restrict__ len, int B, int Tcap, int n_ent,
                                                          int* __restrict__ row_off, int* __restrict__ tiles, int* __restrict__ err) {
  extern __shared__ int sm[];        // off[B + 1] | cnt[1024] | start[1024]
  int* off = sm;
  int* cnt = off + B + 1;
  int* start = cnt + 1024;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int acc = 0;
    for (int b = 0; b < B; ++b) {
      off[b] = min(acc, Tcap);
      acc += len[b];
    }
    off[B] = min(acc, Tcap);
    *err = acc > Tcap ? 1 : 0;
  }
  __syncthreads();
  for (int b = tid; b <= B; b += 1024) row_off[b] = off[b];
  // tiles of 64 rows per row (clamped lengths)
  int c = 0;
  for (int b = 0; b < B; ++b) c += (off[b + 1] - off[b] + VARLEN_TILE - 1) / VARLEN_TILE > tid ? 1 : 0;
  cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int j = 1023; j >= 0; --j) {
      start[j] = acc;
      acc += cnt[j];
    }
    tiles[0] = acc;                  // entries in use
    tiles[1] = off[B];               // T
  }
  __syncthreads();
  int pos = start[tid];
  for (int b = 0; b < B && pos < n_ent; ++b)
    if ((off[b + 1] - off[b] + VARLEN_TILE - 1) / VARLEN_TILE > tid) {
      tiles[2 + 2 * pos] = b;
      tiles[3 + 2 * pos] = tid;
      ++pos;
    }
  __syncthreads();
  const int used = min(start[0] + cnt[0], n_ent);
  for (int e = used + tid; e < n_ent; e += 1024) {
    tiles[2 + 2 * e] = -1;
    tiles[3 + 2 * e] = 0;
  }
}

// per packed token i < Tcap: its row, its position in the row, the shifted decoder input (embed_fwd's `shift` rule) and the target
__global__ __launch_bounds__(256) void pack_tokens_kernel(const int64_t* __restrict__ labels, const int* __restrict__ row_off,
                                                          int B, int L, int Tcap, int start_id, int pad_id,
                                                          int* __restrict__ tok_row, int* __restrict__ tok_pos,
                                                          int64_t* __restrict__ dec_ids, int64_t* __restrict__ targets) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Tcap) return;
  if (i >= row_off[B]) {
    tok_row[i] = -1;
    tok_pos[i] = 0;
    dec_ids[i] = pad_id;
    targets[i] = -100;
    return;
  }
  int lo = 0, hi = B - 1;            // the b with row_off[b] <= i < row_off[b + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (row_off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int t = i - row_off[lo];
  const int64_t* row = labels + (size_t)lo * L;
  int64_t id = t == 0 ? (int64_t)start_id : row[t - 1];
  if (id == -100) id = pad_id;
  tok_row[i] = lo;
  tok_pos[i] = t;
  dec_ids[i] = id;
  targets[i] = row[t];
}

// x[i] = table[ids[i]] + pos[tok_pos[i]], dropout keyed by the packed row (embed_fwd's kernel with the position from tok_pos)
__global__ __launch_bounds__(256) void embed_packed_kernel(const int64_t* __restrict__ ids, const int* __restrict__ tok_pos,
                                                           const float* __restrict__ table, const float* __restrict__ pos,
                                                           float* __restrict__ x, int rows, int d, int vocab, DropCfg dc) {
  DROP_STEP(dc);
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int64_t id = ids[row];
  if (id < 0) id = 0;
  if (id >= vocab) id = vocab - 1;
  const float* trow = table + (size_t)id * d;
  const float* prow = pos + (size_t)tok_pos[row] * d;
  const size_t base = (size_t)row * d;
  for (int col = lane * 4; col < d; col += 256) {
    const f32x4 t4 = *(const f32x4*)(trow + col), p4 = *(const f32x4*)(prow + col);
    float a[4] = {t4[0] + p4[0], t4[1] + p4[1], t4[2] + p4[2], t4[3] + p4[3]};
    if (dc.thresh) {
      float m[4];
      drop_mask4(dc, (base + col) >> 2, m);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] *= m[e];
    }
    *(f32x4*)(x + base + col) = f32x4{a[0], a[1], a[2], a[3]};
  }
}

}  // namespace

extern "C" int mrmt3_pack_lengths(const int64_t* labels, int B, int L, int32_t* len, void* stream) {
  MR_CHECK_ARG(labels && len && B > 0 && L > 0, "pack_lengths: bad args");
  hipLaunchKernelGGL(pack_len_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, L, len);
  MR_CHECK_LAUNCH("pack_lengths");
  return MRMT3_OK;
}

extern "C" int mrmt3_pack_plan(const int64_t* labels, int B, int L, int Tcap, int start_id, int pad_id, int32_t* len,
                               int32_t* row_off, int32_t* tok_row, int32_t* tok_pos, int64_t* dec_ids, int64_t* targets,
                               int32_t* tiles, int32_t* err, void* stream) {
  MR_CHECK_ARG(labels && len && row_off && tok_row && tok_pos && dec_ids && targets && tiles && err, "pack_plan: null pointer");
  MR_CHECK_ARG(B > 0 && L > 0 && Tcap > 0, "pack_plan: bad sizes");
  MR_CHECK_ARG(ceil_div(L, VARLEN_TILE) <= 1024, "pack_plan: rows longer than 65536 tokens");
  const size_t shm = (size_t)(B + 1 + 2048) * sizeof(int);
  MR_CHECK_ARG(shm <= 64 * 1024, "pack_plan: batch too large");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pack_len_kernel, dim3(B), dim3(256), 0, s, labels, L, len);
  hipLaunchKernelGGL(pack_index_kernel, dim3(1), dim3(1024), shm, s, len, B, Tcap, mrmt3_pack_tile_entries(B, Tcap), row_off,
                     tiles, err);
  hipLaunchKernelGGL(pack_tokens_kernel, dim3(ceil_div(Tcap, 256)), dim3(256), 0, s, labels, row_off, B, L, Tcap, start_id,
                     pad_id, tok_row, tok_pos, dec_ids, targets);
  MR_CHECK_LAUNCH("pack_plan");
  return MRMT3_OK;
}

extern "C" int mrmt3_embed_fwd_packed(const int64_t* ids, const int32_t* tok_pos, const float* table, const float* pos, float* x,
                                      int rows, int d, int vocab, float p_drop, uint64_t seed, const int32_t* step_dev,
                                      uint32_t stream_id, void* stream) {
  MR_CHECK_ARG(ids && tok_pos && table && pos && x && rows > 0 && d % 4 == 0, "embed_fwd_packed: bad args");
  hipLaunchKernelGGL(embed_packed_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, ids, tok_pos,
                     table, pos, x, rows, d, vocab, make_drop(p_drop, seed, stream_id, step_dev));
  MR_CHECK_LAUNCH("embed_fwd_packed");
  return MRMT3_OK;
}
