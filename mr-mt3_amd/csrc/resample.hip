// Windowed-sinc resampler at arbitrary ratio that mixes as it goes (mrmt3_resample_mix_fwd): rows of f32 samples
// out of stems resident in one device pool, every source read at its own rate through a polyphase table with linear
// interpolation between neighbouring phases.  The rows then go through mrmt3_logmel_fwd.
//
// One workgroup per (tile of RS_TILE outputs, row); a thread owns RS_R outputs RS_THREADS apart and keeps their row sums in
// registers across the sources, so the mix costs no pass of its own.  Per source the table entries are workgroup-uniform:
// the input span the tile's taps touch is staged into LDS once (zero outside the stem) and every thread walks its taps from
// there, the two coefficient rows of its phase coming from the table in L2 as 16-byte pieces.  A span that does not fit
// (a step above 4, which the host never plans) is read from global memory by the same loop.
//
// The arithmetic is the header's, one rounding per operation, in tap order and in source order: no fused multiply-add, no
// packed f32 (csrc/Makefile), and a tap outside the stem is not added at all (a select, never a product with zero).
#include "common.h"

#pragma clang fp contract(off)

#define RS_THREADS 256
#define RS_R 4                                   // outputs per thread: four independent tap sums in flight
#define RS_TILE (RS_THREADS * RS_R)
#define RS_MAX_TAPS 160
#define RS_MAX_SRC 64
#define RS_PHASES 512                            // ABI constant: a table has RS_PHASES + 1 rows
#define RS_SPAN (RS_TILE * 4 + RS_MAX_TAPS)      // floats of LDS: the span of a full tile at step 4

static MrLaunchCounter g_resample_launches;

typedef float rs_f4 __attribute__((ext_vector_type(4)));
typedef rs_f4 rs_f4a8 __attribute__((aligned(8)));   // a table row starts on 8 bytes (n_taps is even), not on 16

// Taps t .. t + W - 1 (W = 4, or 2 for the last pair of a table whose n_taps is not a multiple of 4) of a thread's RS_R
// outputs.  Every load first, pinned before the first is used: all in flight at once, none sunk into a branch.  The
// coefficient rows are gathered — every lane has a phase of its own — so they are read as wide as the table's alignment
// allows: the launch is bound by the cache lines those gathers touch, and 16 bytes per lane touch half as many as 8.
template <bool LDS, int W>
__device__ __forceinline__ void rs_taps(int t, const float* __restrict__ pool, const float* sm, int T,
                                        const float* const (&h0)[RS_R], const int (&base)[RS_R],
                                        const long long (&first)[RS_R], const int (&tlo)[RS_R], const int (&thi)[RS_R],
                                        const float (&w)[RS_R], float (&acc)[RS_R]) {
  float a[RS_R][W], b[RS_R][W], x[RS_R][W];
#pragma unroll
  for (int r = 0; r < RS_R; ++r) {
    if (W == 4) {
      const rs_f4 va = *(const rs_f4a8*)(h0[r] + t), vb = *(const rs_f4a8*)(h0[r] + T + t);
#pragma unroll
      for (int q = 0; q < W; ++q) { a[r][q] = va[q]; b[r][q] = vb[q]; }
    } else {
      const float2 va = *(const float2*)(h0[r] + t), vb = *(const float2*)(h0[r] + T + t);
      a[r][0] = va.x; a[r][1] = va.y; b[r][0] = vb.x; b[r][1] = vb.y;
    }
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if (LDS) {
        x[r][q] = sm[base[r] + t + q];
      } else {
        // (the index clamped into the stem, which is not empty where a tap is in: what lies outside is loaded from
        // inside and not added)
        const long long i = first[r] + t + q, top = first[r] + thi[r] - 1, bot = first[r] + tlo[r];
        x[r][q] = tlo[r] < thi[r] ? pool[i < bot ? bot : (i > top ? top : i)] : 0.f;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RS_R; ++r)
#pragma unroll
    for (int q = 0; q < W; ++q) asm volatile("" : "+v"(a[r][q]), "+v"(b[r][q]), "+v"(x[r][q]));
#pragma unroll
  for (int r = 0; r < RS_R; ++r) {
#pragma unroll
    for (int q = 0; q < W; ++q) {
      // (the bound pinned behind the previous tap's sum: left alone the scheduler forms all RS_R * W lane masks up front,
      // which is more scalar registers than there are)
      int hi = thi[r];
      asm volatile("" : "+v"(hi), "+v"(acc[r]));
      const bool in = t + q >= tlo[r] && t + q < hi;
      const float d = b[r][q] - a[r][q];
      const float m = w[r] * d;
      const float c = a[r][q] + m;
      const float p = c * x[r][q];
      const float s = acc[r] + p;
      acc[r] = in ? s : acc[r];                // a select: a tap outside the stem is not added
    }
  }
}

// The tap sums of one filtered source for a thread's RS_R outputs, added into `row` with the source's gain.
// first[r]: pool index of tap 0 of output r; taps tlo[r] <= t < thi[r] lie inside the stem (none for an output that is off).
// LDS: sm holds pool[s0 ...] for the whole tile (first[r] - s0 + t is inside it for every t < T).
template <bool LDS>
__device__ __forceinline__ void rs_filtered(const float* __restrict__ pool, const float* sm, long long s0,
                                            const float* __restrict__ h, int T, const long long (&first)[RS_R],
                                            const int (&tlo)[RS_R], const int (&thi)[RS_R], const unsigned (&fr)[RS_R],
                                            float g, float (&row)[RS_R]) {
  float acc[RS_R], w[RS_R];
  const float* h0[RS_R];
  int base[RS_R];
#pragma unroll
  for (int r = 0; r < RS_R; ++r) {
    acc[r] = 0.f;
    w[r] = (float)(fr[r] & 0x7fffffu) * 0x1p-23f;                  // 23 bits: exact
    h0[r] = h + (size_t)(fr[r] >> 23) * T;
    base[r] = LDS ? (int)(first[r] - s0) : 0;
  }
  int t = 0;
  if (LDS) {
    for (; t + 4 <= T; t += 4) rs_taps<LDS, 4>(t, pool, sm, T, h0, base, first, tlo, thi, w, acc);
  }
  for (; t < T; t += 2) rs_taps<LDS, 2>(t, pool, sm, T, h0, base, first, tlo, thi, w, acc);   // (the global reader: pairs only)
#pragma unroll
  for (int r = 0; r < RS_R; ++r) {
    const float v = g * acc[r];
    row[r] = row[r] + v;                       // (an output that is off added nothing: +0, and is written as 0 anyway)
  }
}

__global__ __launch_bounds__(RS_THREADS) void resample_mix_kernel(
    const float* __restrict__ pool, long long pool_samples, const long long* __restrict__ src_pos,
    const long long* __restrict__ src_begin, const long long* __restrict__ src_end, const long long* __restrict__ src_step,
    const float* __restrict__ src_gain, const int* __restrict__ src_filt, int n_src, int batch, int n_samples,
    const float* __restrict__ filt, int n_filt, int T, const long long* __restrict__ valid_samples, float* __restrict__ out,
    int stage) {
  __shared__ float sm[RS_SPAN];
  const int tid = threadIdx.x;
  const int o0 = (int)blockIdx.x * RS_TILE;                              // (< n_samples: an int)
  const int b = (int)(blockIdx.y + blockIdx.z * 65535u);                 // rows on y, and on z past 65535 of them
  if (b >= batch) return;
  {
    long long lim = n_samples;
    if (valid_samples != nullptr && valid_samples[b] < lim) lim = valid_samples[b];
    const int cnt = lim - o0 < RS_TILE ? (lim - o0 < 0 ? 0 : (int)(lim - o0)) : RS_TILE;   // outputs of this tile that sound (uniform)
    float row[RS_R];
#pragma unroll
    for (int r = 0; r < RS_R; ++r) row[r] = 0.f;
    for (int k = 0; cnt > 0 && k < n_src; ++k) {
      // (cnt re-read as an opaque per-lane value in every round: compared once outside the loop, its RS_R lane masks and
      // their complements would sit in scalar registers through all of it)
      int cnt_k = cnt;
      asm volatile("" : "+v"(cnt_k));
      const size_t e = (size_t)b * n_src + k;
      const float g = src_gain[e];
      if (g == 0.0f) continue;                                           // not read at all
      const int f = src_filt[e];
      const long long step = src_step[e], begin = src_begin[e], end = src_end[e];
      if (f < -1 || f >= n_filt || step <= 0 || begin >= end) continue;  // silent
      long long lo = begin < 0 ? 0 : begin, hi = end > pool_samples ? pool_samples : end;
      asm volatile("" : "+v"(lo), "+v"(hi));    // uniform, but compared with per-lane indices only: kept in vector registers
      // 32.32 positions; the products wrap like the int64 arithmetic of the restatement (bounds are checked after it)
      const unsigned long long p0 = (unsigned long long)src_pos[e];
      if (f < 0) {
        // pass-through: pool[n + i], the fraction ignored (mix_source of logmel.hip with a lower bound)
        const long long n0 = (long long)p0 >> 32;
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
          const long long idx = n0 + o0 + tid + r * RS_THREADS;
          if (tid + r * RS_THREADS < cnt_k && idx >= lo && idx < hi) {
            const float v = g * pool[idx];
            row[r] = row[r] + v;
          }
        }
        continue;
      }
      long long first[RS_R];
      int tlo[RS_R], thi[RS_R];
      unsigned fr[RS_R];
      // the tile's span [s0, s0 + len): taps of its first to its last sounding output; staged when the positions do not
      // wrap inside the tile and the span fits
      const long long pos_a = (long long)(p0 + (unsigned long long)o0 * (unsigned long long)step);
      const long long pos_z = (long long)((unsigned long long)pos_a + (unsigned long long)(cnt - 1) * (unsigned long long)step);
      const long long s0 = (pos_a >> 32) - T / 2 + 1;
      const long long len = (pos_z >> 32) + T / 2 + 1 - s0;
      const bool lds = stage != 0 && step <= (4LL << 32) && pos_z >= pos_a && len <= RS_SPAN;
#pragma unroll
      for (int r = 0; r < RS_R; ++r) {
        const bool on = tid + r * RS_THREADS < cnt_k;
        const unsigned long long i = (unsigned)o0 + (unsigned)(tid + r * RS_THREADS);
        const long long pos = on ? (long long)(p0 + i * (unsigned long long)step) : pos_a;
        first[r] = (pos >> 32) - T / 2 + 1;
        fr[r] = (unsigned)(pos & 0xffffffffLL);
        const long long a = lo - first[r], z = hi - first[r];
        tlo[r] = a < 0 ? 0 : (a > T ? T : (int)a);
        thi[r] = !on || z < 0 ? 0 : (z > T ? T : (int)z);
      }
      const float* h = filt + (size_t)f * (RS_PHASES + 1) * T;
      if (lds) {
        __syncthreads();                                                 // the previous source's reads are done
        for (int q = tid; q < (int)len; q += RS_THREADS) {
          const long long idx = s0 + q;
          sm[q] = idx >= lo && idx < hi ? pool[idx] : 0.f;
        }
        __syncthreads();
        rs_filtered<true>(pool, sm, s0, h, T, first, tlo, thi, fr, g, row);
      } else {
        rs_filtered<false>(pool, sm, s0, h, T, first, tlo, thi, fr, g, row);
      }
    }
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const int i = o0 + tid + r * RS_THREADS;                           // (o0 + RS_TILE may pass 2^31: compared unsigned)
      if ((unsigned)i < (unsigned)n_samples) out[(size_t)b * n_samples + (unsigned)i] = tid + r * RS_THREADS < cnt ? row[r] : 0.f;
    }
  }
}

extern "C" int mrmt3_resample_mix_fwd(const float* pool, long long pool_samples, const long long* src_pos,
                                      const long long* src_begin, const long long* src_end, const long long* src_step,
                                      const float* src_gain, const int* src_filt, int n_src, int batch, int n_samples,
                                      const float* filt, int n_filt, int n_taps, const long long* valid_samples, float* out,
                                      void* stream) {
  MR_CHECK_ARG(pool && src_pos && src_begin && src_end && src_step && src_gain && src_filt && filt && out,
               "resample_mix_fwd: null pointer");
  MR_CHECK_ARG(n_src >= 1 && n_src <= RS_MAX_SRC, "resample_mix_fwd: n_src must be in [1, %d], got %d", RS_MAX_SRC, n_src);
  MR_CHECK_ARG(n_taps >= 2 && n_taps <= RS_MAX_TAPS && n_taps % 2 == 0,
               "resample_mix_fwd: n_taps must be even and in [2, %d], got %d", RS_MAX_TAPS, n_taps);
  MR_CHECK_ARG(n_filt >= 0, "resample_mix_fwd: n_filt must be >= 0, got %d", n_filt);
  MR_CHECK_ARG(pool_samples > 0 && batch > 0 && n_samples > 0, "resample_mix_fwd: bad sizes");
  MR_CHECK_ARG(((uintptr_t)filt % 8) == 0, "resample_mix_fwd: filt must be 8-byte aligned");
  // tiles on x (2^31 - 1 of them: n_samples may be a whole stem), rows on y, and on z past 65535 of them
  const dim3 grid((unsigned)(((long long)n_samples + RS_TILE - 1) / RS_TILE), (unsigned)(batch < 65535 ? batch : 65535),
                  (unsigned)((batch + 65534) / 65535));
  // MRMT3_RESAMPLE_LDS=0: every source read from global memory (A/B and parity of the two readers)
  const int stage = MR_KNOB("MRMT3_RESAMPLE_LDS", 1);
  hipLaunchKernelGGL(resample_mix_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, pool, pool_samples, src_pos,
                     src_begin, src_end, src_step, src_gain, src_filt, n_src, batch, n_samples, filt, n_filt, n_taps,
                     valid_samples, out, stage);
  MR_CHECK_LAUNCH("resample_mix_fwd");
  g_resample_launches.hit();
  return MRMT3_OK;
}

extern "C" unsigned long long mrmt3_resample_launches(int reset) { return g_resample_launches.read(reset); }
