// Note matching on the device (mrmt3_note_match_fwd): a maximum-cardinality matching of the bipartite graph
// "reference note ~ estimated note" of contrib/transcription_metrics.match_notes for every problem of one launch; the
// contract is the header's.
//
// One workgroup per problem, three phases behind workgroup barriers, no traffic between workgroups:
//   1. order: every entry of both lists is compared with the valid entry before it; the caller-owned workspace of the
//      problem's entries is cleared (owner of every reference entry, visited stamp, match).
//   2. windows: one thread per estimated entry binary-searches [wlo, whi) in the reference list with the exact onset
//      predicate, which is monotone in the onset: the window is exactly the onset-adjacent references.
//   3. runs: an entry whose wlo is >= its predecessor's whi begins a run; runs share no reference, so they are matched
//      independently.  The waves draw blocks of 64 entries from an LDS counter and a wave matches every run that BEGINS in
//      its block, to the run's end: Kuhn's algorithm with the stack in the workspace.  The 64 lanes test 64 candidates of
//      the current window side by side (pitch, offset, owner, stamp); a ballot picks the first free reference if there is
//      one, else the first unvisited one to descend into.  A run of any length is matched: there is no capacity.
// A run is matched by one wave from its first entry on and in list order, so the matching does not depend on which wave
// drew it: the same bits on every run.
//
// The sides, the clamped list range of a problem and the test of an entry's index are notetab.h's, shared with frames.hip.
//
// f64 work only, one rounding per operation (no fused multiply-add); ordinary vector loads and stores.
#include "notetab.h"

#pragma clang fp contract(off)

#define NM_THREADS 1024
#define NM_WAVE 64

static MrLaunchCounter g_match_launches;

struct NmTol {
  double onset, ratio, offset_min;
};

// what the wave's lanes write is read by its other lanes: workgroup-scope accesses that the compiler keeps in memory
__device__ __forceinline__ int nm_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void nm_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void nm_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

// np.around(|a - b|, 6): multiply, round half to even, divide
__device__ __forceinline__ double nm_dist(double a, double b) {
  return __ddiv_rn(rint(__dmul_rn(fabs(__dsub_rn(a, b)), 1e6)), 1e6);
}

// entry `pos` of a list: does it name a note of the table (note_at) whose onset is a number?
__device__ __forceinline__ bool nm_entry(const NoteSide& s, int pos, int& note, double& on) {
  if (!note_at(s, pos, note)) return false;
  on = s.times[2 * (size_t)note];
  return on == on;
}

// the onset the order and the windows see at `pos`: the entry's, or that of the nearest valid entry before it (an entry
// without a valid index or onset is transparent), -inf if there is none.  `note` receives that entry's index, -1 for none.
__device__ __forceinline__ double nm_key(const NoteSide& s, int first, int pos, int& note) {
  for (int q = pos; q >= first; --q) {
    double on;
    if (nm_entry(s, q, note, on)) return on;
  }
  note = -1;
  return -__builtin_huge_val();
}

__device__ __forceinline__ bool nm_ordered(const NoteSide& s, int first, int pos) {
  int note, before;
  double on;
  if (pos <= first || !nm_entry(s, pos, note, on)) return true;
  const double prev = nm_key(s, first, pos - 1, before);
  return before < 0 || prev < on || (prev == on && before < note);
}

__global__ __launch_bounds__(NM_THREADS) void note_match_kernel(
    NoteSide ref, NoteSide est, const int* __restrict__ prob_flags, int n_prob, const int* __restrict__ pitch_lo,
    const int* __restrict__ pitch_hi, int n_tables, NmTol tol, int* __restrict__ matched, int* match,
    int* __restrict__ status, int* ws) {
  __shared__ int s_bad, s_next, s_matched;
  const int tid = threadIdx.x, lane = tid & (NM_WAVE - 1);
  const int p = blockIdx.x;
  if (p >= n_prob) return;
  int r0, r1, Lr, e0, e1, Le;
  note_range(ref, n_prob, p, r0, r1, Lr);
  note_range(est, n_prob, p, e0, e1, Le);
  const int flags = prob_flags[p];
  const bool offsets = flags & 1;
  const int table = flags >> 8;
  const bool table_ok = table >= 0 && table < n_tables;
  const int* lo_of = pitch_lo + (table_ok ? table : 0) * 128;
  const int* hi_of = pitch_hi + (table_ok ? table : 0) * 128;
  // the workspace: per estimated entry its window and one stack level, per reference entry its owner and its stamp
  int* wlo = ws;
  int* whi = wlo + Le;
  int* stack_e = whi + Le;
  int* stack_r = stack_e + Le;
  int* owner = stack_r + Le;
  int* stamp = owner + Lr;

  if (tid == 0) { s_bad = 0; s_next = 0; s_matched = 0; }
  __syncthreads();
  // ---- 1. order, and the problem's part of the workspace
  bool bad = false;
  for (int q = r0 + tid; q < r1; q += NM_THREADS) {
    owner[q] = -1;
    stamp[q] = 0;
    bad |= !nm_ordered(ref, r0, q);
  }
  for (int k = e0 + tid; k < e1; k += NM_THREADS) {
    match[k] = -1;
    bad |= !nm_ordered(est, e0, k);
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (s_bad) {
    if (tid == 0) { matched[p] = 0; status[p] = 2; }
    return;
  }
  // ---- 2. windows
  for (int k = e0 + tid; k < e1; k += NM_THREADS) {
    int note;
    const double on_e = nm_key(est, e0, k, note);
    // first reference that is not too early: on_r >= on_e or within the tolerance
    int a = r0, b = r1;
    while (a < b) {                              // (at most 32 halvings of r1 - r0)
      const int mid = a + ((b - a) >> 1);
      const double on_r = nm_key(ref, r0, mid, note);
      if (on_r >= on_e || nm_dist(on_r, on_e) <= tol.onset) b = mid; else a = mid + 1;
    }
    const int lo = a;
    // first reference that is too late
    b = r1;
    while (a < b) {
      const int mid = a + ((b - a) >> 1);
      const double on_r = nm_key(ref, r0, mid, note);
      if (on_r > on_e && nm_dist(on_r, on_e) > tol.onset) b = mid; else a = mid + 1;
    }
    wlo[k] = lo;
    whi[k] = a;
  }
  __syncthreads();
  // ---- 3. runs
  int found = 0;                                 // (wave-uniform)
  const int depth_cap = e1 - e0;
  const long long step_cap = 2LL * (r1 - r0) + 2;                       // a root descends once and returns once per reference
  for (;;) {
    int blk = 0;
    if (lane == 0) blk = atomicAdd(&s_next, NM_WAVE);
    blk = __shfl(blk, 0);
    if (blk >= e1 - e0) break;
    const int kb = e0 + blk;
    unsigned long long starts;
    {
      const int k = kb + lane;
      bool start = false;
      if (k < e1) start = k == e0 || wlo[k] >= whi[k - 1];
      starts = __ballot(start);
    }
    while (starts) {
      const int ks = kb + __ffsll((long long)starts) - 1;
      starts &= starts - 1;
      // the run that begins at ks; c_*: the windows of the 64 entries from cb, one per lane
      int cb = ks, c_lo = 0, c_hi = 0;
      bool c_start = false;
      for (int k = ks; k < e1; ++k) {            // (ends at the next run's first entry)
        if (k == ks || k >= cb + NM_WAVE) {
          cb = k;
          const int kk = cb + lane;
          c_start = false;
          if (kk < e1) {
            c_lo = wlo[kk];
            c_hi = whi[kk];
            c_start = kk > ks && c_lo >= whi[kk - 1];
            c_lo = c_lo < r0 ? r0 : c_lo;        // (only an overlapping neighbour's garbage is ever outside)
            c_hi = c_hi > r1 ? r1 : c_hi;
          }
        }
        if (__shfl((int)c_start, k - cb)) break;
        // Kuhn's search from the root k
        const int root_stamp = k - e0 + 1;
        int cur = k, depth = 0;
        int lo = __shfl(c_lo, k - cb), hi = __shfl(c_hi, k - cb);
        for (long long step = 0; step < step_cap; ++step) {
          int note_e;
          double on_e = 0.0, off_e = 0.0;
          int pitch_e = -1;
          const bool e_ok = table_ok && nm_entry(est, cur, note_e, on_e);
          if (e_ok) {
            off_e = est.times[2 * (size_t)note_e + 1];
            pitch_e = est.meta[note_e].x;
          }
          int free_at = -1, down_at = -1;
          for (int base = lo; base < hi && e_ok; base += NM_WAVE) {      // (the window, 64 candidates at a time)
            const int pos = base + lane;
            bool edge = false, is_free = false;
            if (pos < hi) {
              int note_r;
              double on_r;
              if (nm_entry(ref, pos, note_r, on_r)) {
                const double off_r = ref.times[2 * (size_t)note_r + 1];
                const int pitch_r = ref.meta[note_r].x;
                edge = nm_dist(on_r, on_e) <= tol.onset && pitch_r >= 0 && pitch_r < 128;
                if (edge) edge = lo_of[pitch_r] <= pitch_e && pitch_e <= hi_of[pitch_r];
                if (edge && offsets)
                  edge = nm_dist(off_r, off_e) <= fmax(__dmul_rn(tol.ratio, __dsub_rn(off_r, on_r)), tol.offset_min);
              }
              if (edge) {
                const int own = nm_ld(owner + pos);
                is_free = own < 0;
                // an owner is an entry of this problem (anything else: an unordered neighbour wrote here, no edge)
                if (!is_free) edge = own >= e0 && own < e1 && nm_ld(stamp + pos) != root_stamp;
              }
            }
            const unsigned long long fm = __ballot(edge && is_free);
            if (fm) { free_at = base + __ffsll((long long)fm) - 1; break; }
            const unsigned long long dm = __ballot(edge);
            if (dm && down_at < 0) down_at = base + __ffsll((long long)dm) - 1;
          }
          if (free_at >= 0) {                    // flip the path: every entry on the stack takes the reference it went into
            if (lane == 0) {
              int e = cur, r = free_at;
              for (int d = depth;; --d) {
                nm_st(owner + r, e);
                nm_st(match + e, r);
                if (d == 0) break;
                e = nm_ld(stack_e + ks + d - 1);
                r = nm_ld(stack_r + ks + d - 1);
              }
            }
            nm_fence();
            ++found;
            break;
          }
          if (down_at >= 0 && depth + 1 < depth_cap && ks + depth < e1) {
            const int next = nm_ld(owner + down_at);
            if (lane == 0) {
              nm_st(stamp + down_at, root_stamp);
              nm_st(stack_e + ks + depth, cur);
              nm_st(stack_r + ks + depth, down_at);
            }
            nm_fence();
            ++depth;
            cur = next;
          } else {
            if (depth == 0) break;               // no augmenting path from this root
            --depth;
            cur = nm_ld(stack_e + ks + depth);
          }
          cur = __builtin_amdgcn_readfirstlane(cur);
          if (cur < e0 || cur >= e1) break;
          lo = nm_ld(wlo + cur);
          hi = nm_ld(whi + cur);
          lo = lo < r0 ? r0 : lo;
          hi = hi > r1 ? r1 : hi;
        }
      }
    }
  }
  if (lane == 0 && found) atomicAdd(&s_matched, found);
  __syncthreads();
  if (tid == 0) { matched[p] = s_matched; status[p] = 0; }
}

static bool nm_sizes(long long Lr, long long Le) { return Lr >= 0 && Le >= 0 && Lr <= 0x3fffffffLL && Le <= 0x3fffffffLL; }

extern "C" size_t mrmt3_note_match_workspace_bytes(long long Lr, long long Le) {
  if (!nm_sizes(Lr, Le)) return 0;
  return (size_t)(4 * Le + 2 * Lr) * sizeof(int);
}

extern "C" int mrmt3_note_match_fwd(const double* ref_times, const int* ref_meta, long long n_ref_notes,
                                    const double* est_times, const int* est_meta, long long n_est_notes,
                                    const int* ref_idx, const int* ref_first, const int* est_idx, const int* est_first,
                                    const int* prob_flags, int n_prob, const int* pitch_lo, const int* pitch_hi, int n_tables,
                                    double onset_tol, double offset_ratio, double offset_min_tol, int* matched, int* match,
                                    int* status, void* workspace, void* stream) {
  MR_CHECK_ARG(ref_times && ref_meta && est_times && est_meta && ref_idx && ref_first && est_idx && est_first && prob_flags &&
                   pitch_lo && pitch_hi && matched && match && status && workspace,
               "note_match_fwd: null pointer (the workspace too: its size is known to the caller alone)");
  MR_CHECK_ARG(n_prob > 0 && n_tables > 0, "note_match_fwd: n_prob and n_tables must be > 0, got %d, %d", n_prob, n_tables);
  MR_CHECK_ARG(n_tables <= (1 << 22), "note_match_fwd: at most %d pitch tables, got %d", 1 << 22, n_tables);
  NOTETAB_CHECK_COUNTS("note_match_fwd", n_ref_notes, n_est_notes);
  MR_CHECK_ARG(onset_tol >= 0.0 && offset_ratio >= 0.0 && offset_min_tol >= 0.0,
               "note_match_fwd: the tolerances must be >= 0 (a NaN is not), got %g, %g, %g", onset_tol, offset_ratio,
               offset_min_tol);
  NOTETAB_CHECK_META("note_match_fwd", "meta", ref_meta);
  NOTETAB_CHECK_META("note_match_fwd", "meta", est_meta);
  MR_CHECK_ARG(((uintptr_t)workspace % 4) == 0, "note_match_fwd: the workspace must be 4-byte aligned");
  const NoteSide ref{ref_times, (const int4*)ref_meta, n_ref_notes, ref_idx, ref_first};
  const NoteSide est{est_times, (const int4*)est_meta, n_est_notes, est_idx, est_first};
  const NmTol tol{onset_tol, offset_ratio, offset_min_tol};
  hipLaunchKernelGGL(note_match_kernel, dim3((unsigned)n_prob), dim3(NM_THREADS), 0, (hipStream_t)stream, ref, est,
                     prob_flags, n_prob, pitch_lo, pitch_hi, n_tables, tol, matched, match, status, (int*)workspace);
  MR_CHECK_LAUNCH("note_match_fwd");
  g_match_launches.hit();
  return MRMT3_OK;
}

extern "C" unsigned long long mrmt3_note_match_launches(int reset) { return g_match_launches.read(reset); }
