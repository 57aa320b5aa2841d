// Note tables on the device: what the kernels that read one share.  A table is times f64 [n, 2] (onset,
// offset) and meta int32 [n, 4] (pitch, velocity, program | drum << 8, spare), read as one int4; a problem's notes are a
// LIST of table indices, idx[first[p] .. first[p + 1]), and nothing the lists hold is trusted.
#pragma once
#include "common.h"

// one side (reference or estimate) of every problem of a launch
struct NoteSide {
  const double* times;
  const int4* meta;
  long long n_notes;
  const int* idx;
  const int* first;     // [n_prob + 1]
};

// the list range [a, b) of problem p, whatever `first` holds: a in [0, L], b in [a, L], L = max(first[n_prob], 0)
__device__ __forceinline__ void note_range(const NoteSide& s, int n_prob, int p, int& a, int& b, int& L) {
  L = s.first[n_prob];
  L = L < 0 ? 0 : L;
  a = s.first[p];
  b = s.first[p + 1];
  a = a < 0 ? 0 : (a > L ? L : a);
  b = b < a ? a : (b > L ? L : b);
}

// does entry `pos` of the lists name a note of the table?  `note` receives its index as it stands in the list
__device__ __forceinline__ bool note_at(const NoteSide& s, int pos, int& note) {
  note = s.idx[pos];
  return note >= 0 && (long long)note < s.n_notes;
}

// the host checks the entry points share; `who` is the entry point's name, which the text of mrmt3_last_error begins with
#define NOTETAB_CHECK_COUNTS(who, n_ref, n_est)                                                                     \
  MR_CHECK_ARG((n_ref) >= 0 && (n_est) >= 0 && (n_ref) <= 0x7fffffffLL && (n_est) <= 0x7fffffffLL,                  \
               "%s: the note counts must be in [0, 2^31), got %lld, %lld", who, (long long)(n_ref), (long long)(n_est))
#define NOTETAB_CHECK_META(who, what, meta) \
  MR_CHECK_ARG(((uintptr_t)(meta) % 16) == 0, "%s: %s must be 16-byte aligned", who, what)
