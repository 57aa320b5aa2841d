// Frame-level counts and piano rolls from note tables (mrmt3_note_frames_fwd): both sides of every problem of
// one launch are rasterised into bit-packed time x pitch rolls and counted; the contract is the header's.
//
// One unit of work is (problem, tile of NF_TILE frames); the workgroups stride over the units, no traffic between them
// but the integer atomics of the counts:
//   1. the two rolls of the tile are cleared in LDS, [side][128 pitches][NF_TILE / 32] words;
//   2. the threads stride over the problem's two lists; an entry that reaches into the tile is a run of bits in one pitch
//      row: first-word mask, whole words, last-word mask, each an LDS atomic OR.  The workgroup of tile 0 counts the
//      skipped and the clipped entries of the problem;
//   3. after a barrier ref & est, ref and est are pop-counted over the tile, reduced within the wave, and every wave adds
//      its three sums to counts[p] with 64-bit atomics: integers, so the result does not depend on the order.  With `roll`
//      the tile's words are stored as they lie; every word of `roll` belongs to exactly one unit.
// Work is O(entries x tiles) per problem: every unit reads the whole of both lists (profiles/r25_frame_scores.txt).
//
// The sides, the clamped list range of a problem and the test of an entry's index are notetab.h's, shared with match.hip.
//
// f64 work: the two products of the definition, floor and ceil; one rounding per operation (no fused multiply-add);
// ordinary vector loads and stores.
#include "notetab.h"

#pragma clang fp contract(off)

#define NF_THREADS 512
#define NF_WAVE 64
#define NF_TILE 2048                               // frames of a tile: 2 sides x 128 pitches x 64 words = 64 KB of LDS
#define NF_WORDS (NF_TILE / 32)
#define NF_MAX_BLOCKS (1 << 16)

static MrLaunchCounter g_frames_launches;

__device__ __forceinline__ unsigned nf_wave_sum(unsigned v) {
  for (int d = NF_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__global__ __launch_bounds__(NF_THREADS) void note_frames_kernel(NoteSide ref, NoteSide est, int n_prob, double fps,
                                                                  long long n_frames, long long n_tiles, long long W,
                                                                  unsigned long long* __restrict__ counts,
                                                                  int* __restrict__ skipped, int* __restrict__ clipped,
                                                                  unsigned* __restrict__ roll) {
  __shared__ unsigned s_roll[2][128][NF_WORDS];
  const int tid = threadIdx.x, lane = tid & (NF_WAVE - 1);
  const long long units = (long long)n_prob * n_tiles;
  for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int p = (int)(unit / n_tiles);
    const long long tile = unit - (long long)p * n_tiles;
    const long long f0 = tile * NF_TILE;
    const long long f1 = f0 + NF_TILE < n_frames ? f0 + NF_TILE : n_frames;
    int lo[2], hi[2], L;
    for (int s = 0; s < 2; ++s) note_range(s ? est : ref, n_prob, p, lo[s], hi[s], L);
    if (lo[0] == hi[0] && lo[1] == hi[1] && !roll) continue;       // (the same for every thread: no barrier is missed)
    // ---- 1. clear
    for (int i = tid; i < 2 * 128 * NF_WORDS; i += NF_THREADS) (&s_roll[0][0][0])[i] = 0u;
    __syncthreads();
    // ---- 2. the entries
    for (int s = 0; s < 2; ++s) {
      const NoteSide& side = s ? est : ref;
      int n_skip = 0, n_clip = 0;
      for (int q = lo[s] + tid; q < hi[s]; q += NF_THREADS) {
        int note;
        bool ok = note_at(side, q, note);
        double ps = 0.0, pe = 0.0;
        int pitch = 0;
        if (ok) {
          const double start = side.times[2 * (size_t)note], end = side.times[2 * (size_t)note + 1];
          pitch = side.meta[note].x;
          ps = __dmul_rn(start, fps);
          pe = __dmul_rn(end, fps);
          // (a NaN time makes a NaN product, which is not below 2^31 either)
          ok = start == start && end == end && pitch >= 0 && pitch < 128 && ps < 2147483648.0 && pe < 2147483648.0;
        }
        if (!ok) {
          ++n_skip;
          continue;
        }
        const double fa = floor(ps), fb = ceil(pe);
        long long a = fa < 0.0 ? 0 : (long long)fa;                 // (fa may be -inf; it is below 2^31)
        long long b = fb < (double)(a + 1) ? a + 1 : (long long)fb;
        if (b > n_frames) {
          ++n_clip;
          b = n_frames;
        }
        a = a > n_frames ? n_frames : a;
        a = a < f0 ? f0 : a;
        b = b > f1 ? f1 : b;
        if (a >= b) continue;                                       // the entry misses the tile
        const int x = (int)(a - f0), y = (int)(b - f0) - 1;         // bits x .. y of the row, 0 <= x <= y < NF_TILE
        unsigned* row = s_roll[s][pitch];
        const int w0 = x >> 5, w1 = y >> 5;
        const unsigned head = 0xffffffffu << (x & 31), tail = 0xffffffffu >> (31 - (y & 31));
        if (w0 == w1) {
          atomicOr(row + w0, head & tail);
        } else {
          atomicOr(row + w0, head);
          for (int w = w0 + 1; w < w1; ++w) atomicOr(row + w, 0xffffffffu);
          atomicOr(row + w1, tail);
        }
      }
      if (tile == 0) {                                              // (the same for every thread of the workgroup)
        const unsigned sk = nf_wave_sum((unsigned)n_skip), cl = nf_wave_sum((unsigned)n_clip);
        if (lane == 0 && sk) atomicAdd(skipped + 2 * (size_t)p + s, (int)sk);
        if (lane == 0 && cl) atomicAdd(clipped + 2 * (size_t)p + s, (int)cl);
      }
    }
    __syncthreads();
    // ---- 3. count, and the tile's words
    unsigned tp = 0, nr = 0, ne = 0;
    const int words = (int)((f1 - f0 + 31) >> 5);                   // words of the tile that hold a frame
    for (int i = tid; i < 128 * NF_WORDS; i += NF_THREADS) {
      const int pitch = i / NF_WORDS, w = i % NF_WORDS;
      const unsigned r = s_roll[0][pitch][w], e = s_roll[1][pitch][w];
      tp += __popc(r & e);
      nr += __popc(r);
      ne += __popc(e);
      if (roll && w < words) {
        const size_t at = ((size_t)p * 2 * 128 + pitch) * (size_t)W + (size_t)(f0 >> 5) + w;
        roll[at] = r;
        roll[at + 128 * (size_t)W] = e;
      }
    }
    tp = nf_wave_sum(tp);
    nr = nf_wave_sum(nr);
    ne = nf_wave_sum(ne);
    if (lane == 0) {
      if (tp) atomicAdd(counts + 3 * (size_t)p, (unsigned long long)tp);
      if (nr) atomicAdd(counts + 3 * (size_t)p + 1, (unsigned long long)nr);
      if (ne) atomicAdd(counts + 3 * (size_t)p + 2, (unsigned long long)ne);
    }
    __syncthreads();                                                // the next unit clears what this one still reads
  }
}

extern "C" size_t mrmt3_note_frames_workspace_bytes(int n_prob, long long n_frames) {
  (void)n_prob;
  (void)n_frames;
  return 0;                                        // the rolls of a tile live in LDS
}

extern "C" int mrmt3_note_frames_fwd(const double* ref_times, const int* ref_meta, long long n_ref_notes,
                                     const double* est_times, const int* est_meta, long long n_est_notes,
                                     const int* ref_idx, const int* ref_first, const int* est_idx, const int* est_first,
                                     int n_prob, double fps, long long n_frames, long long* counts, int* skipped, int* clipped,
                                     unsigned* roll, void* workspace, void* stream) {
  (void)workspace;
  MR_CHECK_ARG(ref_times && ref_meta && est_times && est_meta && ref_idx && ref_first && est_idx && est_first && counts &&
                   skipped && clipped,
               "note_frames_fwd: null pointer (only roll and the workspace may be null)");
  MR_CHECK_ARG(n_prob > 0, "note_frames_fwd: n_prob must be > 0, got %d", n_prob);
  MR_CHECK_ARG(fps > 0.0 && fps <= 1.7976931348623157e308, "note_frames_fwd: fps must be finite and > 0, got %g", fps);
  MR_CHECK_ARG(n_frames >= 1 && n_frames <= 0x7fffffffLL - 63,
               "note_frames_fwd: n_frames must be in [1, 2^31 - 64], got %lld", n_frames);
  NOTETAB_CHECK_COUNTS("note_frames_fwd", n_ref_notes, n_est_notes);
  NOTETAB_CHECK_META("note_frames_fwd", "meta", ref_meta);
  NOTETAB_CHECK_META("note_frames_fwd", "meta", est_meta);
  hipStream_t st = (hipStream_t)stream;
  MR_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)n_prob * 3 * sizeof(long long), st));
  MR_CHECK_HIP(hipMemsetAsync(skipped, 0, (size_t)n_prob * 2 * sizeof(int), st));
  MR_CHECK_HIP(hipMemsetAsync(clipped, 0, (size_t)n_prob * 2 * sizeof(int), st));
  const long long n_tiles = (n_frames + NF_TILE - 1) / NF_TILE, W = (n_frames + 31) / 32;
  const long long units = (long long)n_prob * n_tiles;
  const unsigned blocks = (unsigned)(units < NF_MAX_BLOCKS ? units : NF_MAX_BLOCKS);
  const NoteSide ref{ref_times, (const int4*)ref_meta, n_ref_notes, ref_idx, ref_first};
  const NoteSide est{est_times, (const int4*)est_meta, n_est_notes, est_idx, est_first};
  hipLaunchKernelGGL(note_frames_kernel, dim3(blocks), dim3(NF_THREADS), 0, st, ref, est, n_prob, fps, n_frames, n_tiles, W,
                     (unsigned long long*)counts, skipped, clipped, roll);
  MR_CHECK_LAUNCH("note_frames_fwd");
  g_frames_launches.hit();
  return MRMT3_OK;
}

extern "C" unsigned long long mrmt3_note_frames_launches(int reset) { return g_frames_launches.read(reset); }
