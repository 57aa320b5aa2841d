// Helpers shared by the attention kernels (attention.hip: forward, two-pass backward, exact-f32 kernels;
// attention_onepass.hip: the one-pass backward): fragment reads, the swizzled LDS tile image and its LDS-DMA fill, the
// attention-probability dropout generator, the launch parameter block, and what the flash kernels share: the row prologue
// (attn_locate), the pair passes (attn_pass_tile), the K/V staging of forward and dQ (kv_stage / kv_prime / kv_step).
#pragma once
#include "common.h"
#include "lds_dma.h"

#define HD 64          // head dim (d_kv)

__device__ __forceinline__ bf16x8 cat8(s16x4 lo, s16x4 hi) {
  return bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
  const u32x4 r = {pack_bf2(lo[0], lo[1]), pack_bf2(lo[2], lo[3]), pack_bf2(hi[0], hi[1]), pack_bf2(hi[2], hi[3])};
  return __builtin_bit_cast(bf16x8, r);      // four v_cvt_pk_bf16_f32 (pairs), nothing to join
}

// attention-probability dropout.  Element (q,k) of head-matrix bh takes byte (k & 3) of the 32-bit word
// W(bh, q, k >> 2) = mix24(seed + bh*CB + q*CQ + (k >> 2)*CK): one mix per query row and group of four consecutive keys.
// Forward and dQ hold exactly such a group per lane and accumulator tile (query on the lane, keys 4g..4g+3 in the four
// registers): ONE mix per 4 elements, the lane's part of the argument is loop-invariant and the key tile's part a scalar.
// dK/dV hold the transposed group (key on the lane, four consecutive queries): the four lanes of a quad hold the same
// four queries for keys 4g..4g+3, so each computes the word of ONE query and reads the other three through DPP
// quad-permutes (a v_and with the lane's byte mask as the DPP instruction, then a compare with the threshold shifted into
// that byte).  Round 2 used 2x2 groups — two mixes per 4 elements in every layout — and the mask was 42-53 % of the
// kernels' vector instructions (profiles/r03_attn_isa_mix.txt).  The drop probability is quantised to thresh8/256
// (p=0.1 -> 26/256) and the keep scale is 256/(256-thresh8), so forward and backward stay exactly consistent and
// unbiased.  The kernels only ZERO the dropped probabilities in the loop; the constant keep scale is applied once to
// the accumulated O / dV (and inside the fused multiply-add that forms dS).  oracle/dropout_ref.attn_keep_mask restates
// the generator; tests compare the kernels' kept sets with it bit for bit and check its statistics on the CPU.
struct AttnDrop {
  const int* step;   // nullable device step counter (see DropCfg::step)
  unsigned seed;
  unsigned thresh8;  // 0 = off
  float scale;
};
#define DROP_CQ 0x9E3779B1u
#define DROP_CK 0x85EBCA6Bu
#define DROP_CB 0xC2B2AE35u
__host__ inline AttnDrop make_attn_drop(float p, unsigned long long seed, unsigned stream, const int* step) {
  AttnDrop d;
  d.step = p > 0.f ? step : nullptr;
  d.seed = ((unsigned)seed ^ (unsigned)(seed >> 32)) + stream * 0x27D4EB2Fu;
  if (p <= 0.f) { d.thresh8 = 0; d.scale = 1.f; }
  else {
    d.thresh8 = (unsigned)(p * 256.0f + 0.5f);
    if (d.thresh8 > 255) d.thresh8 = 255;
    d.scale = 256.0f / (256.0f - (float)d.thresh8);
  }
  return d;
}
// VALU and MFMA do not overlap on a gfx950 SIMD (profiles/tools/coissue_probe.hip), so every instruction of
// the mask costs kernel time.  32-bit integer multiplies are quarter rate; v_mul_u32_u24 is full rate, and
// with the xor-shifts folding the high bits down first the two 24-bit multiplies mix just as well here
// (byte histograms, keep rate and neighbour correlations checked against the 32-bit finaliser).
__device__ __forceinline__ unsigned mix24(unsigned x) {
  x ^= x >> 16; x = __umul24(x, 0x7feb35u); x ^= x >> 15; x = __umul24(x, 0x6ca68bu);
  return x;
}
// byte `byte` (0..3, a compile-time constant: an SDWA byte select on the compare) of the group's word decides element `byte`
__device__ __forceinline__ float drop_sel(const AttnDrop& d, unsigned g, int byte, float v) {
  return ((g >> (8 * byte)) & 0xFFu) >= d.thresh8 ? v : 0.f;
}
// dK/dV layout: word of query r of the lane's quad, fetched from the lane that computed it (quad_perm [r,r,r,r])
template <int R>
__device__ __forceinline__ unsigned quad_word(unsigned w) {
  return (unsigned)__builtin_amdgcn_mov_dpp((int)w, R * 0x55, 0xF, 0xF, true);
}
// ... and the quad's mask applied to the lane's four probabilities and four dP values.  `w` is this lane's word: query (fp-th of
// its quad's four), key group key >> 2; the lane's own element sits in byte (key & 3) = fp of every word of the quad:
// bmask = 0xFF << 8 fp, bthr = thresh8 << 8 fp.
__device__ __forceinline__ void drop_quad(unsigned w, unsigned bmask, unsigned bthr, float (&pk)[4], float (&dk_)[4]) {
  const bool k0_ = (quad_word<0>(w) & bmask) >= bthr, k1_ = (quad_word<1>(w) & bmask) >= bthr;
  const bool k2_ = (quad_word<2>(w) & bmask) >= bthr, k3_ = (quad_word<3>(w) & bmask) >= bthr;
  pk[0] = k0_ ? pk[0] : 0.f; dk_[0] = k0_ ? dk_[0] : 0.f;
  pk[1] = k1_ ? pk[1] : 0.f; dk_[1] = k1_ ? dk_[1] : 0.f;
  pk[2] = k2_ ? pk[2] : 0.f; dk_[2] = k2_ ? dk_[2] : 0.f;
  pk[3] = k3_ ? pk[3] : 0.f; dk_[3] = k3_ ? dk_[3] : 0.f;
}
// max over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48): gfx950's v_permlane16/32_swap are
// plain VALU moves, so the reduction has no LDS (ds_bpermute) round trip in the softmax's dependency chain
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float rows_max(float v) {
  unsigned u = __float_as_uint(v);
  u32x2_t r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  u = __float_as_uint(fmaxf(__uint_as_float(r.x), __uint_as_float(r.y)));
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r.x), __uint_as_float(r.y));
}
// Epilogue rows, widened (the guide's T21: per-lane 8-byte row stores are issue-bound, 16 quarter-lines per instruction).
// A lane holds, of ONE output row, the four 8-byte chunks c[dt] = features 16 dt + 4 fg .. + 3 (the MFMA accumulator
// layout with the row on the lane).  Two v_permlane16_swap per chunk pair trade chunks between the lane groups fg and
// fg ^ 1, after which a lane owns 16 contiguous bytes twice: out[p] = features 32 p + widen_off(fg) .. + 7.  A store
// instruction then writes 64 contiguous bytes per row instead of 32, and a row takes two instructions instead of four.
__device__ __forceinline__ void widen_rows(const u32x2 c[4], u32x4 out[2]) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const u32x2_t r0 = __builtin_amdgcn_permlane16_swap(c[2 * p].x, c[2 * p + 1].x, false, false);
    const u32x2_t r1 = __builtin_amdgcn_permlane16_swap(c[2 * p].y, c[2 * p + 1].y, false, false);
    out[p] = u32x4{r0.x, r1.x, r0.y, r1.y};
  }
}
__device__ __forceinline__ int widen_off(int fg) { return (fg & 1) * 16 + (fg >> 1) * 8; }
// the gradient kernels' 8-byte row stores: accumulator tile dt of the lane's row -> bf16 features 16 dt + 4 fg .. + 3 of `row`
__device__ __forceinline__ void store_row_bf16(bf16_t* row, int dt, int fg, f32x4 a) {
  *(u32x2*)(row + dt * 16 + fg * 4) = u32x2{pack_bf2(a[0], a[1]), pack_bf2(a[2], a[3])};
}
#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f

struct AttnParams {
  const bf16_t *q, *k, *v, *o, *d_o;
  // low half of the f32 attention output, bf16(O - bf16(O)): written by the forward next to `out` when the caller
  // keeps the tape, read back by the dQ kernel so that delta = rowsum(dO * O) sees O to ~16 bits.  With delta taken
  // from the bf16-rounded O alone, dP - delta loses the exact cancellation of whatever the value rows have in common
  // (dS_ij = P_ij dO_i.(V_j - O_i)): q/k weight gradients were 3x further from the fp32 gradient than the
  // reference's own bf16-autocast run (tests/golden/bf16_bound.npz), the v/o gradients were not.
  const bf16_t* o_lo_in;
  bf16_t* o_lo_out;
  bf16_t *out, *dq, *dk, *dv;
  float* lse;
  float* delta;
  int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  int B, H, Lq, Lk, causal;
  int tile_mode;     // (tuning) attn_tile: low nibble = flip shift (0 = none), bit 4 = zigzag order inside a group
  AttnDrop drop;
};

// Variable-length (packed) rows, built on the device by mrmt3_pack_plan (pack.hip).  Row b of the batch owns packed rows
// [row_off[b], row_off[b+1]); packed rows [T, Tcap) with T = row_off[B] are the tail.  `tiles` is the launch list of the varlen
// kernels: tiles[0] = entries in use, tiles[1] = T, then n_ent (row, 64-row tile) pairs, heaviest causal tile first (tile index
// descending), row = -1 for a surplus entry.  n_ent = mrmt3_pack_tile_entries(B, Tcap) = ceil(Tcap/64) + B + 1 depends on the
// shapes alone (a captured launch replays for any batch with the same Tcap) and always leaves at least ceil((Tcap-T)/64) surplus
// entries: those write the tail rows' zeros.
#define VARLEN_TILE 64
struct AttnVarlen {
  const int* row_off;
  const int* tiles;
  int n_ent, Tcap;
};
// VL, the layout parameter of the attention kernel templates: 0 dense rows (a dense launch passes AttnVarlen{}), 1 packed
// self-attention (queries and keys packed), 2 packed cross-attention (queries packed, keys dense); only the prologue differs
// surplus entry e of a varlen launch -> the 64 tail rows it zeroes: [r0, r1)
__device__ __forceinline__ bool varlen_tail_rows(const AttnVarlen& V, int e, int& r0, int& r1) {
  const int k = e - V.tiles[0], T = V.tiles[1];
  r0 = T + k * VARLEN_TILE;
  r1 = min(r0 + VARLEN_TILE, V.Tcap);
  return k >= 0 && r0 < r1;
}
// zero rows [r0, r1) of head h in a [rows][ld] bf16 tensor (workgroup of 256: a 16-byte chunk per thread and pass)
__device__ __forceinline__ void varlen_zero_rows(bf16_t* base, int ld, int h, int r0, int r1) {
  if (!base) return;
  for (int i = threadIdx.x; i < (r1 - r0) * 8; i += 256)
    *(u32x4*)(base + (size_t)(r0 + (i >> 3)) * ld + h * HD + (i & 7) * 8) = u32x4{0u, 0u, 0u, 0u};
}

// ---- LDS tiles: [rows][64] bf16 = 128-B rows, the 16-B chunk index XOR-ed with (row & 7).  Tiles are
// filled by buffer_load ... lds (memory -> LDS, no VGPR round trip, see blds_rows8 below): one wave-instruction
// covers 8 rows x 128 B linearly, so the swizzle is applied to each lane's SOURCE chunk.  The same image
// serves ds_read_b128 row reads and ds_read_b64_tr_b16 transposed reads, both conflict-free.
// Rows past the end of the tensor are zero-filled by the buffer bounds check (their scores are masked).
__device__ __forceinline__ bf16x8 lds_row8(const unsigned char* tile, int row, int c) {
  return *(const bf16x8*)(tile + row * 128 + ((c ^ (row & 7)) << 4));
}
// transposed fragment: rows {row..row+3 via the lane's fq} and +16, chunk c, 8-byte half `sub`
__device__ __forceinline__ bf16x8 lds_tr8(const unsigned char* tile, int row, int c, int sub) {
  const unsigned char* a = tile + row * 128 + ((c ^ (row & 7)) << 4) + sub;
  return cat8(lds_tr16(a), lds_tr16(a + 16 * 128));
}

// Workgroups are dispatched round-robin over the 8 XCDs (linear id % 8) and each XCD has its own L2.  All tiles
// of one (batch, head) stream the same K/V (or Q/dO) rows, so they are made to run on ONE XCD, back to back:
// XCD x takes the contiguous range [x*n/8, (x+1)*n/8) of the (b, h, tile) space, tile fastest.  Without this the
// 8 query tiles of a head land on 8 different XCDs and every one of them pulls K/V through the fabric again.
__device__ __forceinline__ void attn_tile(int& tile, int& h, int& b, int mode) {
  const int nt = gridDim.x, H = gridDim.y;
  const int n = nt * H * (int)gridDim.z;
  int w = blockIdx.x + nt * (blockIdx.y + H * blockIdx.z);
  if ((n & 7) == 0) w = (w & 7) * (n >> 3) + (w >> 3);
  tile = w % nt;
  const int bh = w / nt;
  // A small causal launch (12 segments: 576 unpaired workgroups for 768 slots) is resident all at once, and the
  // dispatcher deals an XCD's workgroups over its 32 CUs in rounds: with tile = j % 8 a CU gets the SAME tile index in
  // every round — 2-3 x 16 key tiles on some CUs, 2-3 x 2 on others.  Every other round of 32 (mode & 15 = 5) takes its
  // tiles in descending order instead, so a CU's workgroups are (t, nt-1-t).  Measured on the decoder self-attention,
  // forward / backward: 8 segments 35.8 -> 28.1 / 91.9 -> 76.8 us, 12 segments 47.5 -> 39.5 / 117.4 -> 106.4, 16
  // segments 49.2 -> 41.2 / 135.4 -> 120.0; from 22 segments the tiles run paired (equal work) and nothing changes.
  // Other round lengths (8, 16, 64) and a zigzag order inside a group were no better (MRMT3_ATTN_TILE_MODE, tuning).
  // (whole (batch, head) groups flip — the position of the group's first tile in its XCD's share decides, a function of
  // bh alone — so the map stays a bijection for any nt, H, B)
  if (mode & 16) tile = (tile & 1) ? nt - 1 - (tile >> 1) : (tile >> 1);
  if (mode & 32) tile = nt - 1 - tile;
  if ((mode & 15) && ((((bh * nt) % ((n & 7) == 0 ? (n >> 3) : n)) >> (mode & 15)) & 1) != 0) tile = nt - 1 - tile;
  h = bh % H;
  b = bh / H;
}
// causal launches pair the 128-row tiles (see the kernels): ceil(n/2) workgroups along x — when that still leaves a few
// workgroups per CU.  A small batch (12 segments x 6 heads: 288 pairs for 512-768 resident workgroup slots) runs the
// tiles unpaired instead: twice the workgroups, unequal (2..16 key tiles each) but all resident at once.
static inline bool attn_paired(int L, int causal, int H, int B) {
  const int n = ceil_div(L, 128);
  return causal && n >= 2 && ((n + 1) / 2) * H * B >= 512;
}
// Small launches (12 segments per GPU: 72 (batch, head) pairs) do not fill the chip with 128-row tiles — the encoder's
// self-attention is 144 workgroups, the decoder's 576 unequal ones for 768 slots: such launches run 64-row tiles
// (16 rows per wave, RT = 1 instantiations) instead, twice the workgroups.  MRMT3_ATTN_FINE=0 / 1 forces it (tuning).
static inline bool attn_fine(int L, bool paired, int causal, int H, int B) {
  if (paired || L <= 64) return false;
  const int e = MR_KNOB("MRMT3_ATTN_FINE", -1);             // (tests switch it: mrmt3_set_knob)
  if (e == 0 || e == 1) return e == 1;
  // causal launches that are too small to pair (up to 21 segments) have unequal tiles: the finer grain balances them
  // (20 segments: forward 54.8 -> 50.0 us, backward 148.4 -> 131.2 us); equal tiles only while the chip is underfilled
  // (cross-attention forward at 16-32 segments is 7-10 % slower with 64-row tiles)
  return causal || (long long)ceil_div(L, 128) * H * B < 768;
}
static inline int attn_grid_x(int L, bool paired) {
  const int n = ceil_div(L, 128);
  return paired ? (n + 1) / 2 : n;
}
// K/V (Q/dO) tiles are staged with buffer_load ... lds: the per-lane byte offset inside an 8-row group is constant
// for the whole kernel, the tile offset is a scalar, and rows past the end of the tensor (or a whole tile that is
// switched off by an out-of-range scalar offset) come back as zeros without touching memory — so the loop needs no
// address arithmetic, no row clamp and no branch around the prefetch.
// (LDS_DMA_OOB, lds_dma.h, is that out-of-range scalar offset.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows_rsrc(const bf16_t* base, int nrows, int ld) {
  return lds_dma_rsrc(base, (size_t)(((nrows - 1) * ld + HD) * 2));
}
__device__ __forceinline__ unsigned rows8_lane_off(int ld, int lane) {     // row lane>>3, swizzled 16-B chunk
  return (unsigned)(((lane >> 3) * ld + (((lane & 7) ^ (lane >> 3)) << 3)) * 2);
}
__device__ __forceinline__ void blds_rows8(__amdgpu_buffer_rsrc_t r, unsigned lane_off, int tile_byte_off, unsigned char* dst) {
  lds_dma16(r, dst, lane_off, tile_byte_off);
}

// ---- the prologue of the flash kernels (attention.hip), written once: which (batch) row, head and tile the workgroup owns, the
// row's lengths and its base offsets.  VL = 0: the grid and attn_tile.  VL = 1 / 2: entry blockIdx.x / H of the tile list for
// head blockIdx.x % H; a surplus entry calls zero_tail(h, r0, r1) for the tail rows [r0, r1) it owns and the workgroup is done
// (attn_locate returns false).  KEY_TILES (the dK/dV kernel, a workgroup owns keys): packed self-attention takes the list in
// reverse (key tile t of a causal row is seen by the queries from 64 t on: the low tiles are the heavy ones), packed
// cross-attention keeps the dense grid over the Lk keys of every row and an empty row (Lq = 0) gets st0 = 0 (it reads no
// statistics; keep the address inside the buffer).
struct AttnRow {
  int tile, h, b;
  int Lq, Lk;
  size_t qr0, kr0;            // first row of this (batch) row's queries / keys
  size_t st0;                 // first lse / delta element of this (row, head)
};
template <int VL, bool KEY_TILES = false, typename ZeroTail>
__device__ __forceinline__ bool attn_locate(const AttnParams& P, const AttnVarlen& V, AttnRow& R, ZeroTail&& zero_tail) {
  if constexpr (VL == 0 || (VL == 2 && KEY_TILES)) {
    attn_tile(R.tile, R.h, R.b, P.tile_mode);
  } else {
    const int w = blockIdx.x / P.H;
    const int e = KEY_TILES ? V.n_ent - 1 - w : w;
    R.h = blockIdx.x % P.H;
    R.b = V.tiles[2 + 2 * e];
    R.tile = V.tiles[3 + 2 * e];
    if (R.b < 0) {
      int r0, r1;
      if (varlen_tail_rows(V, e, r0, r1)) zero_tail(R.h, r0, r1);
      return false;
    }
  }
  if constexpr (VL == 0) {
    R.Lq = P.Lq; R.Lk = P.Lk;
    R.qr0 = (size_t)R.b * R.Lq; R.kr0 = (size_t)R.b * R.Lk;
    R.st0 = ((size_t)R.b * P.H + R.h) * R.Lq;
  } else {
    const int o0 = V.row_off[R.b];
    R.Lq = V.row_off[R.b + 1] - o0;
    R.qr0 = (size_t)o0;
    if constexpr (VL == 1) { R.Lk = R.Lq; R.kr0 = R.qr0; }
    else { R.Lk = P.Lk; R.kr0 = (size_t)R.b * P.Lk; }
    R.st0 = (size_t)R.h * V.Tcap + o0;
    if constexpr (KEY_TILES) R.st0 = R.Lq > 0 ? R.st0 : 0;
  }
  return true;
}
// causal launches pair the 128-row tiles: a workgroup takes tiles (n-1-t, t) in two passes — query tile t needs 2(t+1) key tiles
// (key tile t is seen by the queries from 128 t on), so every workgroup of the launch does the same amount of work and the
// launch has no tail of heavy tiles.  far_first: pass 0 takes n-1-t.  Returns false when pass 1 has nothing left (odd n: the
// middle tile is its own partner); pass 1 starts once every wave is done reading the previous tile's LDS stages.
template <bool PAIR>
__device__ __forceinline__ bool attn_pass_tile(int pass, int tile, int n, bool far_first, int& t) {
  t = tile;
  if (PAIR) {
    t = (pass == 0) == far_first ? n - 1 - tile : tile;
    if (pass == 1 && 2 * tile == n - 1) return false;
    if (pass == 1) __syncthreads();
  }
  return true;
}

// ---- K/V staging of the forward and dQ kernels: 64-key tiles, KV_STAGES LDS stages of K tile | V tile, two tiles in flight.
#define KV_STAGES 3
#define KV_STAGE_BYTES 16384   // K tile 8 KiB + V tile 8 KiB
struct KvSrc {
  __amdgpu_buffer_rsrc_t kres, vres;
  unsigned k_lane, v_lane;
  int ldk, ldv;
};
__device__ __forceinline__ KvSrc kv_src(const bf16_t* kb, const bf16_t* vb, int Lk, int ldk, int ldv, int lane) {
  return KvSrc{rows_rsrc(kb, Lk, ldk), rows_rsrc(vb, Lk, ldv), rows8_lane_off(ldk, lane), rows8_lane_off(ldv, lane), ldk, ldv};
}
// each wave (uw) stages 16 rows of K and of V per tile (2 + 2 wave-instructions); `on` = false turns the tile into
// four zero-fills that never leave the CU, which keeps the vmcnt arithmetic of the loop uniform
__device__ __forceinline__ void kv_stage(unsigned char* lds, const KvSrc& S, int uw, int buf, int kv0, bool on) {
  unsigned char* base = lds + buf * KV_STAGE_BYTES;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int t = uw * 2 + i;
    blds_rows8(S.kres, S.k_lane, on ? (kv0 + t * 8) * S.ldk * 2 : LDS_DMA_OOB, base + t * 1024);
    blds_rows8(S.vres, S.v_lane, on ? (kv0 + t * 8) * S.ldv * 2 : LDS_DMA_OOB, base + 8192 + t * 1024);
  }
}
// before the loop: tiles 0 and 1
__device__ __forceinline__ void kv_prime(unsigned char* lds, const KvSrc& S, int uw, int n_kv) {
  kv_stage(lds, S, uw, 0, 0, true);
  kv_stage(lds, S, uw, 1, 64, n_kv > 1);
}
// top of iteration j (`cur` = its stage, 0 at j = 0): wait for tile j, prefetch tile j + 2 into the stage tile j - 1 left,
// rotate `cur`; returns tile j's K image, its V image follows at + 8192.  After the loop VMCNT(0): the switched-off
// prefetches of the last two iterations still write their zeros.
__device__ __forceinline__ const unsigned char* kv_step(unsigned char* lds, const KvSrc& S, int uw, int& cur, int j, int n_kv) {
  VMCNT(4);                                       // tile j landed (tile j+1 may still be in flight)
  __builtin_amdgcn_s_barrier();
  kv_stage(lds, S, uw, cur == 0 ? 2 : cur - 1, j * 64 + 128, j + 2 < n_kv);
  const unsigned char* lk = lds + cur * KV_STAGE_BYTES;
  cur = cur == KV_STAGES - 1 ? 0 : cur + 1;
  return lk;
}

// attention_onepass.hip: the backward in one pass when a workgroup can own all keys of a (batch, head); 1 = launched
int mrmt3_attn_bwd_onepass_try(const AttnParams& P, hipStream_t s);

// attention_general.hip: exact-f32 arithmetic on f32 / bf16 operands, optional additive bias and its gradient
int mrmt3_attn_general_fwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* bias,
                           long long bias_bs, void* o, int ldo, float* lse, int B, int H, int Lq, int Lk, int causal,
                           int dtype, const AttnDrop& drop, hipStream_t s);
int mrmt3_attn_general_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o, int ldo,
                           const void* d_o, int lddo, const float* lse, float* delta, const float* bias, long long bias_bs,
                           void* dq, int lddq, void* dk, int lddk, void* dv, int lddv, float* dbias, int B, int H, int Lq,
                           int Lk, int causal, int dtype, const AttnDrop& drop, hipStream_t s);
// attention_general.hip: the varlen exact-f32 kernels (Lk > 0: dense cross-attention keys [B][Lk]; Lk = 0: packed self keys)
int mrmt3_attn_general_fwd_varlen(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                                  float* lse, const int* row_off, int B, int H, int Tcap, int Lmax, int Lk, int causal,
                                  const AttnDrop& drop, hipStream_t s);
int mrmt3_attn_general_bwd_varlen(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* o,
                                  int ldo, const void* d_o, int lddo, const float* lse, float* delta, void* dq, int lddq,
                                  void* dk, int lddk, void* dv, int lddv, const int* row_off, int B, int H, int Tcap, int Lmax,
                                  int Lk, int causal, const AttnDrop& drop, hipStream_t s);
