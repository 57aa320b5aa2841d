// The ping-pong K loop of the second-generation GEMMs (gemm8.hip: NT, gemm_tn8.hip: TN), once.
//
// What round 1's kernel left on the table (profiles/r01_pmc_gemm_sq.txt: waves parked on s_waitcnt / s_barrier 39 %,
// MFMA pipe busy ~30 %) was its schedule — one barrier per K step, the fragment reads of a step starting only behind
// that barrier, two workgroup-wide stages — not its traffic.  These kernels are built around the schedule instead:
//
//   * 512 threads = 8 waves = 2 per SIMD; the two waves of a SIMD (wave w and w + 4: "group" 0 and 1) run the SAME
//     program one s_barrier apart, so while one of them issues its 16 MFMAs of a phase the other reads fragments
//     from LDS and issues the next LDS-DMA loads (ping-pong; MI355X_MICROARCH "two waves per SIMD").  pp_prologue()
//     puts group 1 one barrier behind, pp_exit() pairs that barrier off at the end.
//   * a 256 x 256 (NT also 128 x 256) tile, K step 64, two LDS buffers of four 16-KiB half-tiles each.
//     A half-tile is what ONE phase reads: HA0 / HA1 = the first / second half of every wave's rows, HB0 / HB1 the
//     first / second half of every wave's columns.  A K step is four phases of 16 (8) MFMAs per wave:
//         ph1 reads HA0, HB0   (r0 x c0)      ph2 reads HB1   (r0 x c1)
//         ph3 reads HA1        (r1 x c1)      ph4 reads none  (r1 x c0)
//     and every phase issues ONE half-tile of LDS-DMA (buffer_load ... lds) two K steps ahead, into the slot whose
//     last reader finished two phases ago:
//         ph1: HB1(u+1) -> buf ^ 1   ph2: HA1(u+1) -> buf ^ 1   ph3: cursor to u+2, HA0(u+2) -> buf   ph4: HB0(u+2) -> buf.
//     Each load therefore has ~5 phases to land, and the only wait in the loop is a counted vmcnt that leaves the
//     four youngest half-tiles in flight (never 0), placed one phase before the half-tile is read: in ph1 for HB1,
//     in ph2 for HA1, in ph4 for HA0 / HB0 of the next K step; ph3 waits for nothing.
//   * a phase = a read segment (fragment reads, the kernel's global stores if it has any, the phase's LDS-DMA request,
//     the counted wait), PP_SEG_END, the MFMAs, PP_MMA_END.  The partner group runs its MFMAs beside the read segment.
//   * a thread's piece of a half-tile is 1 KiB per wave-instruction at wave * PP_PIECE, further ones PP_STRIDE apart.
//
// pp_kstep() below is that K step: phase order, load targets and the places of the waits are stated THERE for both
// kernels.  A kernel hands in its own operations (fragment reads, requests, MFMAs, load cursor, stores, wait counts).
//
// (Tried: issuing a phase's LDS-DMA requests between its MFMAs instead of in the read segment.  A wave issues in
// order and an LDS-DMA instruction takes 60+ cycles to issue, so the MFMAs behind it wait: barriers + MFMAs alone
// went from 1.03 to 1.30 us per K step.  In the read segment the same issue time runs beside the partner's MFMAs.)
// (Tried, not kept: all 160 KiB of LDS — a third B buffer, B requested three K steps ahead, 7 instead of 4 half-tiles
// in flight per CU.  Same results, 917 against 945 TF over the step's shapes: the K loop is not waiting for bytes in
// flight.  A side lesson of that variant: when the K-step body grew a second lambda, hipcc stopped inlining it, the
// accumulators it captures by reference went to scratch memory and the kernel ran 50x slower.  Hence: pp_kstep and
// every lambda handed to it carry __attribute__((always_inline)).)
// (In the TN kernel the transposed fragment reads must be inline asm, or hipcc drains vmcnt in every phase: see
// t8_frag in gemm_tn8.hip.)
#pragma once
#include "lds_dma.h"

#define PP_HALF 16384              // one half-tile
#define PP_BUF (4 * PP_HALF)       // one buffer: HA0, HA1, HB0, HB1
#define PP_PIECE 1024              // a wave-instruction's piece of a half-tile
#define PP_STRIDE 8192             // between a thread's pieces (8 waves x PP_PIECE)
#define PP_INLINE __attribute__((always_inline))

// end of a read segment: the partner's MFMAs are over (barrier), this wave's fragments have arrived, MFMAs run at priority
#define PP_SEG_END()                            \
  __builtin_amdgcn_sched_barrier(0);            \
  __builtin_amdgcn_s_barrier();                 \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
  __builtin_amdgcn_sched_barrier(0);            \
  __builtin_amdgcn_s_setprio(1)
#define PP_MMA_END()                            \
  __builtin_amdgcn_s_setprio(0);                \
  __builtin_amdgcn_sched_barrier(0);            \
  __builtin_amdgcn_s_barrier();                 \
  __builtin_amdgcn_sched_barrier(0)

// K steps 0 and (half of) 1 requested, HA0(0) / HB0(0) landed, group 1 (waves 4-7) set one barrier behind group 0.
// load_a / load_b (buf, half) request a half-tile at the load cursor, cursor_next() moves the cursor one K step on.
template <class LA, class LB, class NEXT, class WAIT>
__device__ PP_INLINE void pp_prologue(int group, LA& load_a, LB& load_b, NEXT& cursor_next, WAIT& wait_first) {
  load_a(0, 0); load_b(0, 0); load_b(0, 1); load_a(0, 1);
  cursor_next();
  load_a(1, 0); load_b(1, 0);
  wait_first();                                              // four half-tiles may stay in flight behind HA0(0), HB0(0)
  __builtin_amdgcn_s_barrier();
  if (group == 1) __builtin_amdgcn_s_barrier();
}

// The switched-off requests of the last K steps still write their zeros; group 0 pairs off group 1's extra barrier.
__device__ __forceinline__ void pp_exit(int group) {
  VMCNT(0);
  if (group == 0) __builtin_amdgcn_s_barrier();
}

// One K step on buffer BUF.  read_a / read_b (buf, half): fragment reads; mma(rh, ch): the MFMAs of row half rh x
// column half ch; stores(ph): the global stores of phase ph's read segment (ph = 1 .. 4); wait(ph): the counted wait
// of phase ph (ph = 1, 2, 4).
template <int BUF, class RA, class RB, class LA, class LB, class MMA, class NEXT, class ST, class WAIT>
__device__ PP_INLINE void pp_kstep(RA& read_a, RB& read_b, LA& load_a, LB& load_b, MMA& mma, NEXT& cursor_next,
                                   ST& stores, WAIT& wait) {
  // ph1: r0 x c0
  read_a(BUF, 0);
  read_b(BUF, 0);
  stores(1);
  load_b(BUF ^ 1, 1);
  wait(1);                                                   // HB1 of this K step (read in ph2)
  PP_SEG_END();
  mma(0, 0);
  PP_MMA_END();
  // ph2: r0 x c1
  read_b(BUF, 1);
  stores(2);
  load_a(BUF ^ 1, 1);
  wait(2);                                                   // HA1 of this K step (read in ph3)
  PP_SEG_END();
  mma(0, 1);
  PP_MMA_END();
  // ph3: r1 x c1
  read_a(BUF, 1);
  stores(3);
  cursor_next();
  load_a(BUF, 0);
  PP_SEG_END();
  mma(1, 1);
  PP_MMA_END();
  // ph4: r1 x c0
  stores(4);
  load_b(BUF, 0);
  wait(4);                                                   // HA0, HB0 of the next K step
  PP_SEG_END();
  mma(1, 0);
  PP_MMA_END();
}

// The f32 epilogues hold, per lane, 4 columns of row r (lanes 0-7 of a 16-lane row) or r + 8 (lanes 8-15: `up`) in each
// of two neighbouring column tiles lo / hi.  The lanes of rows r and r + 8 exchange halves (DPP row_ror:8), after which a
// store instruction writes 8 rows x 128 contiguous bytes (whole lines) instead of 16 rows x 64: v1 goes to row r, v2 to
// row r + 8, at column offset (up ? 16 : 0) + 4 * (lane / 16) of the pair.
__device__ __forceinline__ void pp_exchange_f32(f32x4 lo, f32x4 hi, bool up, f32x4& v1, f32x4& v2) {
  const f32x4 send = up ? lo : hi;
  f32x4 recv;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    recv[e] = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send[e]), 0x128, 0xf, 0xf, false));
  v1 = up ? recv : lo;
  v2 = up ? hi : recv;
}
// The same on packed bf16 words: `keep` is the half the lane stores for its own row, `send` the half its partner stores.
__device__ __forceinline__ void pp_exchange_bf16(u32x4 keep, u32x4 send, bool up, u32x4& v1, u32x4& v2) {
  u32x4 recv;
#pragma unroll
  for (int e = 0; e < 4; ++e) recv[e] = (unsigned)__builtin_amdgcn_mov_dpp((int)send[e], 0x128, 0xf, 0xf, false);   // row_ror:8
  v1 = up ? recv : keep;
  v2 = up ? keep : recv;
}
