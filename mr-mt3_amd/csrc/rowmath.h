// The arithmetic of the row kernels, once.
//
// A fused launch promises the SAME BITS as the two kernels it replaces (mrmt3_gemm_nt_addnorm / _normbwd / _geglubwd /
// _geglu against mrmt3_gemm_nt + the row kernel).  The one decision behind that promise — the order of the f32
// operations and where the dropout mask goes in — is written down here and nowhere else: rowops.hip (the stand-alone row
// kernels), gemm_rows.hip (the row phases of the fused projection kernels) and gemm8.hip (the gated-GELU epilogue) inline
// these functions, so the two forms are equal by construction and the bitwise tests only confirm it.  The functions work
// on values in registers: no global or LDS access (but for the typed 4-wide load / store family at the top) and no
// shuffles — a wave reduction stays with its caller, which hands in and gets back the per-lane partial sums.  Each body
// switches contraction off, like the activation helpers of common.h: every a * b + c meant as an FMA is an explicit fmaf
// and nothing else may fuse, whatever the including file's setting is.
#pragma once
#include "common.h"

// ---- typed 4-wide load / store (16 bytes of f32, 8 bytes of bf16) ---------------------------------------------------------
__device__ __forceinline__ void unpack4(f32x4 t, float v[4]) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
__device__ __forceinline__ void unpack4(u32x2 t, float v[4]) {
  v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xFFFF0000u);
  v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xFFFF0000u);
}
__device__ __forceinline__ void unpack8(u32x4 t, float v[8]) {
  unpack4(u32x2{t.x, t.y}, v);
  unpack4(u32x2{t.z, t.w}, v + 4);
}
__device__ __forceinline__ u32x4 pack8(const float v[8]) {
  return u32x4{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
}
template <typename T> struct Raw4;                       // what 4 elements of T are in memory
template <> struct Raw4<float> {
  typedef f32x4 type;
  static __device__ __forceinline__ f32x4 pack(const float v[4]) { return f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct Raw4<bf16_t> {
  typedef u32x2 type;
  static __device__ __forceinline__ u32x2 pack(const float v[4]) { return u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])}; }
};
template <typename T> __device__ __forceinline__ void load4(const T* p, float v[4]) {
  unpack4(*(const typename Raw4<T>::type*)p, v);
}
template <typename T> __device__ __forceinline__ void store4(T* p, const float v[4]) {
  *(typename Raw4<T>::type*)p = Raw4<T>::pack(v);
}
// streaming (non-temporal) forms: for operands a kernel reads once and nobody reads again soon (the saved activations of
// the backward), and for outputs whose reader is several kernels away (the residual stream) — they then do not push
// the tensors the NEXT kernel wants out of the 256 MB Infinity Cache
template <typename T> __device__ __forceinline__ void load4_nt(const T* p, float v[4]) {
  unpack4(__builtin_nontemporal_load((const typename Raw4<T>::type*)p), v);
}
template <typename T> __device__ __forceinline__ void store4_nt(T* p, const float v[4]) {
  __builtin_nontemporal_store(Raw4<T>::pack(v), (typename Raw4<T>::type*)p);
}

// ---- dropout: v *= keep-scale of the quad idx4 (elements 4 idx4 .. + 3 of the site), nothing when dropout is off ------------
__device__ __forceinline__ void mask4(const DropCfg& d, unsigned long long idx4, float v[4]) {
#pragma clang fp contract(off)
  if (d.thresh) {
    float m[4];
    drop_mask4(d, idx4, m);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= m[e];
  }
}
// the quads q0 and q0 + 1: both masks first, then the eight products (fewer VCC hazard waits than two mask4 in a row)
__device__ __forceinline__ void mask8(const DropCfg& d, unsigned long long q0, float v[8]) {
#pragma clang fp contract(off)
  if (d.thresh) {
    float m[8];
    drop_mask4(d, q0, m);
    drop_mask4(d, q0 + 1, m + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= m[e];
  }
}

// ---- residual add + dropout + T5LayerNorm, forward --------------------------------------------------------------------------
// v += dropout(y) (y is masked in place): the residual stream, which the caller stores if it wants; then ss + sum v^2 in
// element order
__device__ __forceinline__ void norm_fwd_add(const DropCfg& dy, unsigned long long idx4, float v[4], float y[4]) {
#pragma clang fp contract(off)
  mask4(dy, idx4, y);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] += y[e];
}
__device__ __forceinline__ float norm_fwd_sumsq(const float v[4], float ss) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) ss = fmaf(v[e], v[e], ss);
  return ss;
}
// ss: the row's sum of squares, reduced over the wave
__device__ __forceinline__ float norm_rstd(float ss, float cols, float eps) {
#pragma clang fp contract(off)
  return rsqrtf(ss / cols + eps);
}
// o = w * (v * rstd), masked when the site drops its output
__device__ __forceinline__ void norm_fwd_out(const float w[4], const float v[4], float rstd, const DropCfg& dout, int out_drop,
                                             unsigned long long idx4, float o[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = w[e] * (v[e] * rstd);
  if (out_drop) mask4(dout, idx4, o);
}

// ---- the same norm, backward ----------------------------------------------------------------------------------------------
// in: g = dxn, xh = x1.  out: xh = x1 * rstd, g = dxn * w; dwp += dxn * xh; returns dot + sum g * xh (element order)
__device__ __forceinline__ float norm_bwd_acc(float g[4], float xh[4], const float w[4], float rstd, float dwp[4], float dot) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    xh[e] *= rstd;
    dwp[e] = fmaf(g[e], xh[e], dwp[e]);
    g[e] *= w[e];
    dot = fmaf(g[e], xh[e], dot);
  }
  return dot;
}
// dot: the row's sum, reduced over the wave
__device__ __forceinline__ float norm_bwd_mean(float dot, float cols) {
#pragma clang fp contract(off)
  return dot / cols;
}
// one element of dx1 = rstd * (g - xh * mean); then add4 of the residual gradient when there is one, then the masked bf16 copy
// for dy is mask4 on the sum.  (Per element: with the quad as an out-parameter the 2048-column stand-alone kernel with a bf16
// dxn came out at 256 VGPRs instead of 231, one workgroup per CU instead of two.)
__device__ __forceinline__ float norm_bwd_dx(float g, float xh, float rstd, float mean) {
#pragma clang fp contract(off)
  return rstd * fmaf(-xh, mean, g);
}
__device__ __forceinline__ void add4(float d[4], const float r[4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] += r[e];
}

// ---- gated GELU (HF T5DenseGatedGeluDense + NewGELUActivation), 8 elements = the quads q0 and q0 + 1 of g ---------------
__device__ __forceinline__ void geglu_fwd8(const DropCfg& d, unsigned long long q0, const float a[8], const float b[8], float o[8]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = gelu_new_f(a[e]) * b[e];
  mask8(d, q0, o);
}
// go = dg is masked in place; da / db = the gradients of the two halves of h
__device__ __forceinline__ void geglu_bwd8(const DropCfg& d, unsigned long long q0, const float a[8], const float b[8], float go[8],
                                           float da[8], float db[8]) {
#pragma clang fp contract(off)
  mask8(d, q0, go);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float f, fd;
    gelu_new_fd(a[e], &f, &fd);
    da[e] = go[e] * b[e] * fd;
    db[e] = go[e] * f;
  }
}
