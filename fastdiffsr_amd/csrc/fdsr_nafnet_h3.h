// The fp32-grade f16x3 form of naf_gemm_kernel (FDSR_PREC_F16X3), included by fdsr_nafnet.hip: same GemmArgs, same tile
// (BM pixels x BN packed columns, 4 waves of 32 pixels x 64 columns), same prologues and epilogues; only the products change.
//   * the staged activation -- fp32 after LN + FiLM or after the SCA multiply -- is clamped to +-65504 and split in registers into
//     hi = f16(a), lo = f16(a - hi); a value beyond the range (or a NaN) raises the sticky flag GemmArgs::sat first (a plain vector store)
//   * the weights arrive pre-split (split_weights: hi / lo planes of w 2^e in B-fragment order, straight from L2 into VGPRs)
//   * every product is lo.hi + hi.lo + hi.hi on v_mfma_f32_32x32x16_f16 into the fp32 accumulator, chunk after chunk in k order:
//     one summation order per output, no split-K, no atomics; the accumulator is un-scaled by 2^-e (exact) before the bias
// Operand / accumulator maps, the clamp before the split and the power-of-two weight scale are those of fdsr_conv_h.hip.
// LDS: one row per pixel, [32 k hi | 32 k lo | 16 B pad] = 144 B (nine 16-byte slots, odd: the operand's ds_read_b128 over
// consecutive pixel rows lands on distinct slots), two buffers, one barrier per chunk.
#pragma once

typedef _Float16 naf_h8 __attribute__((ext_vector_type(8)));

constexpr int HK = 32;                // k per staged chunk: two 32x32x16 steps
constexpr int HROW = 2 * HK * 2 + 16; // LDS bytes per pixel row
constexpr float F16_MAX = 65504.f;

template <int PRO, bool VEC>
__global__ void __launch_bounds__(NT) naf_gemm_h3_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char sA[2][BM * HROW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int HWo = p.Hout * p.Wout;
  const int M = p.N * HWo;
  const int m0 = blockIdx.x * BM, co0 = blockIdx.y * BN;

  // thread t stages pixel t % BM, k in [16 (t / BM), +16) of every chunk
  const int am = t & (BM - 1), ak = (t >> 7) * 16;
  const int gm = m0 + am;
  const bool mval = gm < M;
  int n = 0, oy = 0, ox = 0;
  if (mval) {
    n = gm / HWo;
    const int r = gm - n * HWo;
    oy = r / p.Wout;
    ox = r - oy * p.Wout;
  }
  const int iy0 = oy * p.S - p.P, ix0 = ox * p.S - p.P;
  float mean = 0.f, rstd = 0.f;
  const float *pm = nullptr, *pa = nullptr;
  if (PRO != PRO_NONE && mval) {
    pm = p.pmul + (size_t)n * p.pstride;
    if (PRO == PRO_LN) {
      pa = p.padd + (size_t)n * p.pstride;
      mean = p.stats[2 * (size_t)gm];
      rstd = p.stats[2 * (size_t)gm + 1];
    }
  }

  float ra[16];
  auto load = [&](int kc) {
    const int kb = kc * HK + ak;
    if (!VEC) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = kb + j;
        float v = 0.f;
        if (mval && k < p.K) {
          const int tap = k / p.Cin, ci = k - tap * p.Cin;
          const int ky = tap / p.KW, kx = tap - ky * p.KW;
          const int iy = iy0 + ky, ix = ix0 + kx;
          if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) v = p.x[(((size_t)n * p.Hin + iy) * p.Win + ix) * p.Cin + ci];
        }
        ra[j] = v;
      }
    } else {
#pragma unroll
      for (int o = 0; o < 2; ++o) {   // two octets: each lies inside one tap (Cin % 8 == 0)
        const int k = kb + 8 * o;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (mval && k < p.K) {
          const int tap = k / p.Cin, ci = k - tap * p.Cin;
          const int ky = tap / p.KW, kx = tap - ky * p.KW;
          const int iy = iy0 + ky, ix = ix0 + kx;
          if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) {
            const f32x4* src = reinterpret_cast<const f32x4*>(p.x + (((size_t)n * p.Hin + iy) * p.Win + ix) * p.Cin + ci);
            v0 = src[0];
            v1 = src[1];
            if (PRO != PRO_NONE) {
              const f32x4 m0v = *reinterpret_cast<const f32x4*>(pm + ci), m1v = *reinterpret_cast<const f32x4*>(pm + ci + 4);
              if (PRO == PRO_LN) {
                const f32x4 a0v = *reinterpret_cast<const f32x4*>(pa + ci), a1v = *reinterpret_cast<const f32x4*>(pa + ci + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  v0[j] = (v0[j] - mean) * rstd * m0v[j] + a0v[j];
                  v1[j] = (v1[j] - mean) * rstd * m1v[j] + a1v[j];
                }
              } else {
                v0 *= m0v;
                v1 *= m1v;
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { ra[8 * o + j] = v0[j]; ra[8 * o + 4 + j] = v1[j]; }
      }
    }
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

  // weight fragments [column tile][chunk][nb][s][plane][lane] x 16 B: element j of lane l is w[k = 32 chunk + 16 s + 8 (l >> 5) + j]
  // [column = 64 tile + 32 nb + (l & 31)] (the 32x32x16 B operand map)
  const int nk = (p.Kpad + HK - 1) / HK;
  const uint4* wq = p.wq + ((size_t)blockIdx.y * nk * 8) * 64 + lane;
  uint4 Bf[2][2][2];
  auto load_b = [&](int kc, int nb, int s) {
    const uint4* src = wq + ((size_t)kc * 8 + nb * 4 + s * 2) * 64;
    Bf[nb][s][0] = src[0];
    Bf[nb][s][1] = src[64];
  };

  f32x16 acc[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;

  const int r31 = lane & 31, h = lane >> 5;
  // 32x32x16 A operand: A[i = lane & 31][k = 8 (lane >> 5) + j] (pixel, k)
  const int aoff = (wave * 32 + r31) * HROW + 16 * h;
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

  // the epilogue of naf_gemm_kernel on acc * winv (no out2: training does not run in this mode)
  // C/D map: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (pixel)
  const float winv = p.winv;
  const int mw = m0 + wave * 32 + 4 * h;
  if (p.epi == EPI_GATE) {
    const int half = p.Cout >> 1;
    const int cg = blockIdx.y * 32 + r31;
    if (cg >= half) return;
    const float b0 = p.bias[co0 + r31], b1 = p.bias[co0 + 32 + r31];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int om = mw + (i & 3) + 8 * (i >> 2);
      if (om >= M) continue;
      const float u0 = acc[0][i] * winv + b0, u1 = acc[1][i] * winv + b1;
      p.out[(size_t)om * p.ostride + cg] = u0 * u1;
    }
    return;
  }
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const int co = co0 + nb * 32 + r31;
    if (co >= p.Cout) continue;
    const float bias = p.bias[co];
    const float ev = p.epi == EPI_RES ? p.evec[co] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int om = mw + (i & 3) + 8 * (i >> 2);
      if (om >= M) continue;
      const float v = acc[nb][i] * winv + bias;
      if (p.epi == EPI_PSHUF) {
        const int pn = om / HWo, r = om - pn * HWo;
        const int y = r / p.Wout, x = r - y * p.Wout;
        const int c = co >> 2, dy = (co >> 1) & 1, dx = co & 1;
        const size_t oi = (((size_t)pn * 2 * p.Hout + 2 * y + dy) * 2 * p.Wout + 2 * x + dx) * p.ostride + c;
        p.out[oi] = v + p.res[oi];
      } else {
        const size_t oi = (size_t)om * p.ostride + co;
        p.out[oi] = p.epi == EPI_RELU ? fmaxf(v, 0.f) : p.epi == EPI_RES ? p.res[oi] + v * ev : v;
      }
    }
  }
}
