// The fp32-grade f16x3 form of naf_gemm_kernel (FDSR_PREC_F16X3), included by fdsr_nafnet.hip after fdsr_nafnet_gemm.h: its k-loop.
//   * the staged activation -- fp32 after LN + FiLM or after the SCA multiply -- is clamped to +-65504 and split in registers into
//     hi = f16(a), lo = f16(a - hi); a value beyond the range (or a NaN) raises the sticky flag GemmArgs::sat first (a plain vector store)
//   * the weights arrive pre-split (split_weights: hi / lo planes of w 2^e in B-fragment order, straight from L2 into VGPRs)
//   * every product is lo.hi + hi.lo + hi.hi on v_mfma_f32_32x32x16_f16 into the fp32 accumulator, chunk after chunk in k order:
//     one summation order per output, no split-K, no atomics; the accumulator is un-scaled by 2^-e (exact) before the bias
// Operand / accumulator maps, the clamp before the split and the power-of-two weight scale are those of fdsr_conv_h.hip.
// LDS: one row per pixel, [32 k hi | 32 k lo | 16 B pad] = 144 B (nine 16-byte slots, odd: the operand's ds_read_b128 over
// consecutive pixel rows lands on distinct slots), two buffers, one barrier per chunk.
#pragma once

constexpr int HROW = 2 * HK * 2 + 16; // LDS bytes per pixel row

template <int PRO, bool VEC>
__global__ void __launch_bounds__(NT) naf_gemm_h3_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char sA[2][BM * HROW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * BM, co0 = blockIdx.y * BN;

  // thread t stages pixel t % BM, k in [16 (t / BM), +16) of every chunk
  const int am = t & (BM - 1), ak = (t >> 7) * 16;
  const NafRow row = naf_row<PRO>(p, m0 + am);

  float ra[16];
  auto load = [&](int kc) {
    const int kb = kc * HK + ak;
    if (VEC) {
      naf_gather_octet<PRO>(p, row, kb, ra);
      naf_gather_octet<PRO>(p, row, kb + 8, ra + 8);
    } else naf_gather_scalar<16>(p, row, kb, ra);
  };
  // range guard, clamp, split, store: [hi k | lo k] of this thread's 16 k
  auto stage = [&](unsigned char* buf) {
    bool out = false;   // beyond the range, infinite or NaN
#pragma unroll
    for (int j = 0; j < 16; ++j) out |= !(fabsf(ra[j]) <= F16_MAX);
    if (out) *p.sat = 1;
    unsigned char* dst = buf + am * HROW + ak * 2;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      naf_h8 hi, lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = __builtin_amdgcn_fmed3f(ra[8 * o + j], -F16_MAX, F16_MAX);
        hi[j] = (_Float16)v;
        lo[j] = (_Float16)(v - (float)hi[j]);
      }
      *reinterpret_cast<naf_h8*>(dst + 16 * o) = hi;
      *reinterpret_cast<naf_h8*>(dst + 2 * HK + 16 * o) = lo;
    }
  };

  const int nk = (p.Kpad + HK - 1) / HK;
  uint4 Bf[2][2][2];   // [nb][s][hi, lo]
  auto load_b = [&](int kc, int nb, int s) {
    const uint4* src = naf_bfrag(p, nk, lane, kc, nb, s);
    Bf[nb][s][0] = src[0];
    Bf[nb][s][1] = src[64];
  };

  f32x16 acc[2];
  naf_zero(acc);

  const int aoff = naf_aoff(lane, wave, HROW);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int s = 0; s < 2; ++s) load_b(0, nb, s);
  load(0);
  stage(sA[0]);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const unsigned char* cur = sA[kc & 1] + aoff;
    const bool more = kc + 1 < nk;
    if (more) load(kc + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const naf_h8 ahi = *reinterpret_cast<const naf_h8*>(cur + 32 * s);
      const naf_h8 alo = *reinterpret_cast<const naf_h8*>(cur + 2 * HK + 32 * s);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, __builtin_bit_cast(naf_h8, Bf[nb][s][0]), acc[nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, __builtin_bit_cast(naf_h8, Bf[nb][s][1]), acc[nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, __builtin_bit_cast(naf_h8, Bf[nb][s][0]), acc[nb], 0, 0, 0);
        if (more) load_b(kc + 1, nb, s);   // same registers, next chunk
      }
    }
    if (more) stage(sA[(kc + 1) & 1]);   // the other buffer: its last readers passed the previous barrier
    __syncthreads();
  }

  naf_epilogue(p, acc, m0, co0, lane, wave, NafEpiF32<true>{p});
}
