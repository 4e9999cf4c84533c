// Device-side pieces of the 16-bit UNet convolutions, written once: fdsr_conv_h.hip, fdsr_conv_k32.hip, fdsr_conv_up2.hip,
// fdsr_conv_strip.hip (all three STRIP_PART builds), fdsr_conv_tail.hip and fdsr_wgrad.hip include it; fdsr_kernels.hip takes the
// block-id remap and the fast SiLU from it.  Internal header, HIP sources only.  Everything here is a type, a __device__
// __forceinline__ function or a template: no kernel, no launch, no state.  The functions are expressions lifted out of the kernels
// as they stood -- each kernel keeps its own k-loop, prefetch schedule, LDS layout and stores, and its A/B switches and timing
// probes stay around the calls.
#pragma once
#include "fdsr_kernels.h"
#include "fdsr_act_io.h"

namespace fdsr {

// ---- register vector types (f32x4 / f32x16: fdsr_act_io.h) ----
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // (native vectors: arrays of HIP's uint4 struct were left in scratch memory)

// x * sigmoid(x) (unet.py:57-59); v_exp_f32 + v_rcp_f32, ~3e-7 relative
__device__ __forceinline__ float silu_fast(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

// Workgroup b of a grid of nwg -> its work item, XCD-contiguous: the hardware deals consecutive workgroups round-robin to the eight
// XCDs, so XCD x gets the items [x's share) in order and neighbouring tiles (shared halo, shared weights) meet in one L2.
__device__ __forceinline__ int xcd_block_id(int b, int nwg) {
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = b & 7, k = b >> 3;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + k;
}

// ---- the f16x3 operand split of a staged quad: clamp to +-lim (65504: the f16 range, NaN-free; 0: the conv's zero padding, in the
// same v_med3), hi = rn_f16(v), lo = rn_f16(v - hi): 22 mantissa bits together.  The two forms give the same bits; a kernel keeps
// the one it was tuned with.  Values come back in registers: the LDS layouts differ per kernel. ----
// mix form: one packed convert and two v_fma_mix per pair, lo = f16(fma(hi, -1, v)) rounded once
__device__ __forceinline__ void split2_mix(float a, float b, float lim, unsigned& hi, unsigned& lo) {
  const float ca = __builtin_amdgcn_fmed3f(a, -lim, lim), cb = __builtin_amdgcn_fmed3f(b, -lim, lim);
  const h2 h = {(_Float16)ca, (_Float16)cb};
  hi = __builtin_bit_cast(unsigned, h);
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(hi), "v"(ca));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(hi), "v"(cb));
}
__device__ __forceinline__ void split4_mix(f32x4 v, float lim, uint2& hi, uint2& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(v[e], -lim, lim);
  {
    const h2 h0 = {(_Float16)v[0], (_Float16)v[1]}, h1 = {(_Float16)v[2], (_Float16)v[3]};
    hi.x = __builtin_bit_cast(unsigned, h0);
    hi.y = __builtin_bit_cast(unsigned, h1);
  }
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lo.x) : "v"(hi.x), "v"(v[0]));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo.x) : "v"(hi.x), "v"(v[1]));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lo.y) : "v"(hi.y), "v"(v[2]));
  asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo.y) : "v"(hi.y), "v"(v[3]));
}
// two-step form: convert, subtract in fp32, convert
__device__ __forceinline__ void split4_2step(f32x4 v, float lim, h4& hi, h4& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(v[e], -lim, lim);
  hi = h4{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
  lo = h4{(_Float16)(v.x - (float)hi.x), (_Float16)(v.y - (float)hi.y), (_Float16)(v.z - (float)hi.z), (_Float16)(v.w - (float)hi.w)};
}

// ---- where K chunk kc (KC channels) of a launch comes from: the concatenated input x0 | x1, or -- chunks nk and up of a RIDER
// launch -- the rider's raw second input xr0 | xr1 (never GroupNorm'ed).  q: this thread's float4 slot within the chunk. ----
struct ChunkSrc {
  const float* base;   // tensor the chunk lies in
  int Cs, cc;          // its channel count; this thread's first channel within it
  int cbase;           // the chunk's first channel within its (concatenated) input
  bool gn;             // GroupNorm scale / shift apply
};
// What a loop knows about the chunks it stages, at compile time: all main chunks, all rider chunks, or either (told apart by
// kc >= nk at run time).  A loop of one kind carries no test of kc: its loads, waits and staging arithmetic are straight-line.
enum ChunkKind { CHUNK_MAIN = 0, CHUNK_RIDER = 1, CHUNK_ANY = 2 };
template <int KIND>
__device__ __forceinline__ bool chunk_is_rider(int kc, int nk) { return KIND == CHUNK_ANY ? kc >= nk : KIND == CHUNK_RIDER; }

template <bool RIDER, int KIND = (RIDER ? CHUNK_ANY : CHUNK_MAIN)>
__device__ __forceinline__ ChunkSrc chunk_src(const ConvParams& p, int kc, int KC, int nk, int q, bool gn) {
  ChunkSrc s;
  s.cbase = kc * KC;
  s.gn = gn;
  if (RIDER && chunk_is_rider<KIND>(kc, nk)) {
    s.cbase -= nk * KC;
    s.gn = false;
    if (s.cbase < p.Cr0) { s.base = p.xr0; s.Cs = p.Cr0; s.cc = s.cbase + q * 4; }
    else { s.base = p.xr1; s.Cs = p.Cr1; s.cc = s.cbase - p.Cr0 + q * 4; }
  } else if (s.cbase < p.C0) { s.base = p.x0; s.Cs = p.C0; s.cc = s.cbase + q * 4; }
  else { s.base = p.x1; s.Cs = p.C1; s.cc = s.cbase - p.C0 + q * 4; }
  return s;
}

// ---- the staged activation: GroupNorm apply, Swish unless `plain` (unet.py:89-101); train-mode Dropout behind it (keep bytes 0 / 1) ----
__device__ __forceinline__ f32x4 gn_act4(f32x4 v, f32x4 sc, f32x4 sh, bool plain) {
  v = v * sc + sh;
  if (!plain) { v.x = silu_fast(v.x); v.y = silu_fast(v.y); v.z = silu_fast(v.z); v.w = silu_fast(v.w); }
  return v;
}
__device__ __forceinline__ f32x4 drop4(f32x4 v, unsigned mask_bytes, float scale) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= (float)((mask_bytes >> (8 * e)) & 0xffu) * scale;
  return v;
}

// ---- epilogue ----
// The additive constant of output channel c: bias (+ the rider's) + noise-embedding shift.  Every load is unconditional: the caller
// clamps c and passes the image's noise-embedding row as tembp with tmul = 1, or a stand-in address (the bias) with tmul = 0.  With
// `if (p.temb)` around the loads the compiler puts an s_waitcnt vmcnt(0) behind each -- exposed round trips at the end of every tile.
// (Plain values, no ConvParams reference: the form that left every kernel's code as it was.)
template <bool RIDER>
__device__ __forceinline__ float epi_add1(const float* bias, const float* bias_r, const float* tembp, float tmul, int c) {
  float a = bias[c];
  if (RIDER) a += bias_r[c];
  a += tmul * tembp[c];
  return a;
}
template <bool RIDER>
__device__ __forceinline__ f32x4 epi_add4(const float* bias, const float* bias_r, const float* tembp, float tmul, int c) {
  f32x4 a;
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = epi_add1<RIDER>(bias, bias_r, tembp, tmul, c + r);
  return a;
}
// four consecutive output channels in the launch's stored type: OUT16 the mode's 16-bit activation format, else fp32
template <int PREC, bool OUT16>
__device__ __forceinline__ void put4(float* out, size_t idx, f32x4 v) {
  if (OUT16) *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(out) + idx) = pack4_16<PREC>(v);
  else *reinterpret_cast<f32x4*>(out + idx) = v;
}

// The part_out / gsum_out tails (the GroupNorm statistics of the output) are NOT here.  conv_mfma_h_kernel / conv_up2_h_kernel and
// conv_k32_kernel / conv_up2_k32_kernel each hold a pair that agrees statement for statement but for the partial's tile index; as one
// function (ConvParams by reference, or every operand by value) the pair changed the register allocation of the kernels around it
// (VGPRs of 68 conv_k32_kernel instantiations, +-1 .. 10; scratch of five), so the four copies stay where they are.  The strip kernel
// (a wave owns its 16 channels: no LDS fold) and the two kernels of fdsr_conv_tail.hip (per-wave partial rows) fold differently anyway.

}  // namespace fdsr
