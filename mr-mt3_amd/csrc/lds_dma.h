// The LDS-DMA primitives of the GEMM and attention kernels (buffer_load ... lds: global memory straight into LDS, no
// registers in between), one copy: the buffer resource, the 16-byte request, the offset that switches a request off, the
// counted wait, the transposed LDS read, the XCD-major workgroup index and the host-side addressing limit.
#pragma once
#include "common.h"

// A scalar offset past every buffer's `bytes`: the request returns zeros into LDS without touching memory, so a loop
// switches a prefetch off (past the last K step, past the last tile) with no branch around it.
#define LDS_DMA_OOB 0x7FFF0000

// Raw buffer over [base, base + bytes): offsets past the end read as zeros (rows past the end of a tensor).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t lds_dma_rsrc(const void* base, size_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
}

// One wave-instruction: lane p's 16 bytes at voff + soff go to dst + 16 p (1 KiB per instruction).
// (Kept in a __device__ function: called from a lambda inside a kernel template, the builtin makes hipcc's host pass
// drop the kernel's launch stub without a diagnostic.)
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t r, unsigned char* dst, unsigned voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
}

// counted wait: all but the n youngest vector-memory requests (LDS-DMA loads and global stores, in order) have completed
#define VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// ds_read_b64_tr_b16: four bf16 of a 16 x 16 block, transposed by the hardware
__device__ __forceinline__ s16x4 lds_tr16(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

// Logical workgroup index of a grid that is a multiple of 8: workgroups with equal blockIdx % 8 share an XCD (and its
// L2), so XCD x takes the contiguous eighth [x n / 8, (x + 1) n / 8) of the work items, in dispatch order.
__device__ __forceinline__ int xcd_major_index() {
  const int per = (int)gridDim.x >> 3;
  return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}

// Host: an operand of `rows` rows of `ld` elements (+ `cols` in the last one), 2 bytes each, lies below the offset
// that switches a request off.  Each launcher passes its own rows / ld / cols (padded or not: they differ on purpose).
static inline bool lds_dma_fits(size_t rows, size_t ld, size_t cols) {
  return (rows * ld + cols) * 2 < (size_t)LDS_DMA_OOB;
}
