// The f16 storage mode of the NAFNet (FDSR_NAF_STORE_F16), included by fdsr_nafnet.hip after fdsr_nafnet_h3.h: every NHWC activation
// between kernels is f16 in memory, every product is one v_mfma_f32_32x32x16_f16 into an fp32 accumulator.  A kernel widens what it
// reads (exact), computes as its fp32 sibling does and rounds once (to nearest even) where it stores; side results formed from
// registers (the strip sums) come from the fp32 values before that rounding.  A value to be stored or staged beyond +-65504 (or a NaN)
// is clamped with fmed3 and raises the sticky flag (a plain vector store), in every kernel that stores f16.
//   naf_gemm_h1_kernel: naf_gemm_kernel's gather, prologues and epilogue walk (fdsr_nafnet_gemm.h) around a k-loop of its own.
//   * the VEC path loads 8 halves (16 B) per octet; with PRO_NONE they go to LDS as they are, otherwise the fp32 value after LN + FiLM
//     or the SCA multiply is rounded to f16 once.  The non-VEC instance (intro) reads the fp32 xin.
//   * the weights are the hi planes of split_weights' fragments, f16(w 2^e), straight from L2 into VGPRs; the accumulator is un-scaled
//     by 2^-e (exact) before the bias.  Chunk after chunk in k order: one summation order per output, no split-K, no atomics.
//   * LDS: one row per pixel, 32 k x 2 B + 16 B pad = 80 B (five 16-byte slots, odd: the operand's ds_read_b128 over consecutive pixel
//     rows lands on distinct slots), two buffers, one barrier per chunk.
//   * the store: the 32x32 C/D map gives a lane one column and 16 rows, 2 B per lane in 64-byte row segments.  After the last barrier
//     the staging LDS is free: the rounded tile is turned through it (144-byte rows) and leaves as 16 B per lane.  PixelShuffle
//     (a scatter) and ending's fp32 eps store directly.
#pragma once

typedef _Float16 naf_h2 __attribute__((ext_vector_type(2)));

constexpr int H1ROW = HK * 2 + 16;   // staging LDS bytes per pixel row
constexpr int H1OP = BN * 2 + 16;    // bytes per pixel row of the output tile in LDS

// the one rounding of a stored value
__device__ __forceinline__ _Float16 naf_to_h(float v, int* sat) {
  if (!(fabsf(v) <= F16_MAX)) *sat = 1;
  return (_Float16)__builtin_amdgcn_fmed3f(v, -F16_MAX, F16_MAX);
}

// epilogue policies (naf_epilogue): res is f16; a finished value goes to global memory (f16, or fp32 under o32), or rounded into the
// LDS tile [pixel row][column] of H1OP-byte rows.  wi: 2^-e, the kernel argument or (training) the device table's.  pair: training
// keeps conv4's pair before the gate as f16 too, [M][Cout] in channel order
struct NafEpiH1 {
  static constexpr bool SCALE = true;
  const GemmArgs& p;
  float wi;
  __device__ __forceinline__ float winv() const { return wi; }
  __device__ __forceinline__ float res(size_t oi) const { return (float)reinterpret_cast<const _Float16*>(p.res)[oi]; }
  __device__ __forceinline__ void put(size_t oi, int, int, float v) const {
    if (p.o32) p.out[oi] = v;
    else reinterpret_cast<_Float16*>(p.out)[oi] = naf_to_h(v, p.sat);
  }
  __device__ __forceinline__ void pair(int om, int cg, float u0, float u1) const {
    if (!p.out2) return;
    _Float16* o = reinterpret_cast<_Float16*>(p.out2);
    o[(size_t)om * p.Cout + cg] = naf_to_h(u0, p.sat);
    o[(size_t)om * p.Cout + (p.Cout >> 1) + cg] = naf_to_h(u1, p.sat);
  }
};
struct NafEpiH1Lds : NafEpiH1 {
  unsigned char* tile;
  __device__ __forceinline__ void put(size_t, int row, int col, float v) const {
    *reinterpret_cast<_Float16*>(tile + row * H1OP + col * 2) = naf_to_h(v, p.sat);
  }
};

template <int PRO, bool VEC>
__global__ void __launch_bounds__(NT) naf_gemm_h1_kernel(GemmArgs p) {
  static_assert(BM * H1OP <= 2 * BM * H1ROW, "the output tile fits the staging buffers");
  __shared__ __attribute__((aligned(16))) unsigned char sA[2 * BM * H1ROW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * BM, co0 = blockIdx.y * BN;
  const _Float16* xh = reinterpret_cast<const _Float16*>(p.x);   // VEC: the input is f16

  // thread t stages pixel t % BM, k in [16 (t / BM), +16) of every chunk
  const int am = t & (BM - 1), ak = (t >> 7) * 16;
  const NafRow row = naf_row<PRO>(p, m0 + am);

  // what a chunk's loads leave in registers; the arithmetic waits until stage(), after the MFMAs of the chunk before
  float rf[VEC ? 1 : 16];
  naf_h8 rh[2];
  f32x4 rm[2][2], rd[2][2];
  bool ok[2];
  auto load = [&](int kc) {
    const int kb = kc * HK + ak;
    if constexpr (!VEC) naf_gather_scalar<16>(p, row, kb, rf);
    else {
#pragma unroll
      for (int o = 0; o < 2; ++o) {   // two octets: each lies inside one tap (Cin % 8 == 0)
        int ci;
        size_t off;
        ok[o] = naf_tap(p, row, kb + 8 * o, ci, off);
#pragma unroll
        for (int j = 0; j < 8; ++j) rh[o][j] = (_Float16)0.f;
        if (ok[o]) {
          rh[o] = *reinterpret_cast<const naf_h8*>(xh + off);
          if (PRO != PRO_NONE) {
            rm[o][0] = *reinterpret_cast<const f32x4*>(row.pm + ci);
            rm[o][1] = *reinterpret_cast<const f32x4*>(row.pm + ci + 4);
            if (PRO == PRO_LN) {
              rd[o][0] = *reinterpret_cast<const f32x4*>(row.pa + ci);
              rd[o][1] = *reinterpret_cast<const f32x4*>(row.pa + ci + 4);
            }
          }
        }
      }
    }
  };
  // prologue in fp32, range guard, clamp, one rounding, store: this thread's 16 k
  auto stage = [&](unsigned char* buf) {
    unsigned char* dst = buf + am * H1ROW + ak * 2;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      naf_h8 q = rh[o];
      if (!VEC || PRO != PRO_NONE) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (!VEC) v[j] = rf[VEC ? 0 : 8 * o + j];
          else if (!ok[o]) v[j] = 0.f;
          else v[j] = naf_pro<PRO>((float)rh[o][j], row.mean, row.rstd, rm[o][j >> 2][j & 3], PRO == PRO_LN ? rd[o][j >> 2][j & 3] : 0.f);
        }
        bool out = false;   // beyond the range, infinite or NaN
#pragma unroll
        for (int j = 0; j < 8; ++j) out |= !(fabsf(v[j]) <= F16_MAX);
        if (out) *p.sat = 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (_Float16)__builtin_amdgcn_fmed3f(v[j], -F16_MAX, F16_MAX);
      }
      *reinterpret_cast<naf_h8*>(dst + 16 * o) = q;
    }
  };

  const int nk = (p.Kpad + HK - 1) / HK;
  uint4 Bf[2][2];   // the hi plane only
  auto load_b = [&](int kc, int nb, int s) { Bf[nb][s] = *naf_bfrag(p, nk, lane, kc, nb, s); };

  f32x16 acc[2];
  naf_zero(acc);

  const int aoff = naf_aoff(lane, wave, H1ROW);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int s = 0; s < 2; ++s) load_b(0, nb, s);
  load(0);
  stage(sA);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const unsigned char* cur = sA + (kc & 1) * (BM * H1ROW) + aoff;
    const bool more = kc + 1 < nk;
    if (more) load(kc + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const naf_h8 a = *reinterpret_cast<const naf_h8*>(cur + 32 * s);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(naf_h8, Bf[nb][s]), acc[nb], 0, 0, 0);
        if (more) load_b(kc + 1, nb, s);   // same registers, next chunk
      }
    }
    if (more) stage(sA + ((kc + 1) & 1) * (BM * H1ROW));   // the other buffer: its last readers passed the previous barrier
    __syncthreads();
  }

  const float wi = p.winvp ? *p.winvp : p.winv;
  if (p.epi == EPI_PSHUF || p.o32) {
    naf_epilogue(p, acc, m0, co0, lane, wave, NafEpiH1{p, wi});
    return;
  }
  // rounded values into LDS [pixel row][column of the tile], then 16 B per lane: a row's 8-column octets are whole (Cout % 8 == 0)
  naf_epilogue(p, acc, m0, co0, lane, wave, NafEpiH1Lds{{p, wi}, sA});
  __syncthreads();
  const int M = p.N * p.Hout * p.Wout;
  const bool gate = p.epi == EPI_GATE;
  const int cvalid = gate ? p.Cout >> 1 : p.Cout;   // columns of `out`
  const int cbase = gate ? blockIdx.y * 32 : co0;   // the tile's first
  const int octs = gate ? 4 : 8;                    // 16-byte pieces per row
  _Float16* outh = reinterpret_cast<_Float16*>(p.out);
  for (int idx = t; idx < BM * octs; idx += NT) {
    const int r = idx / octs, oc = idx - r * octs;
    if (m0 + r >= M || cbase + 8 * oc >= cvalid) continue;
    *reinterpret_cast<naf_h8*>(outh + (size_t)(m0 + r) * p.ostride + cbase + 8 * oc) = *reinterpret_cast<const naf_h8*>(sA + r * H1OP + oc * 16);
  }
}

// ---- the small kernels' f16 forms: the fp32 siblings' arithmetic on widened values, vector loads (c % 8 == 0 past intro) ----

// naf_ln_stats_kernel: 16 lanes per pixel, 8 channels per load
__global__ void __launch_bounds__(256) naf_ln_stats_h_kernel(const _Float16* __restrict__ x, float* __restrict__ stats, int M, int C) {
  const int sub = threadIdx.x & 15;
  const int pix = blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool ok = pix < M;
  const _Float16* row = x + (size_t)(ok ? pix : 0) * C;
  float s = 0.f;
  for (int c = sub * 8; c < C; c += 128) {
    const naf_h8 v = *reinterpret_cast<const naf_h8*>(row + c);
    s += (((float)v[0] + (float)v[1]) + ((float)v[2] + (float)v[3])) + (((float)v[4] + (float)v[5]) + ((float)v[6] + (float)v[7]));
  }
#pragma unroll
  for (int o = 8; o; o >>= 1) s += __shfl_xor(s, o, 16);
  const float mean = s / (float)C;
  float q = 0.f;
  for (int c = sub * 8; c < C; c += 128) {
    const naf_h8 v = *reinterpret_cast<const naf_h8*>(row + c);
    float d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = (float)v[j] - mean;
    q += ((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) + ((d[4] * d[4] + d[5] * d[5]) + (d[6] * d[6] + d[7] * d[7]));
  }
#pragma unroll
  for (int o = 8; o; o >>= 1) q += __shfl_xor(q, o, 16);
  if (ok && sub == 0) {
    stats[2 * (size_t)pix] = mean;
    stats[2 * (size_t)pix + 1] = 1.f / sqrtf(q / (float)C + LN_EPS);
  }
}

// naf_dw_gate_kernel: a lane owns two neighbouring channels (4-byte loads); LP = 2^lp_shift >= min(64, c / 2) lanes cover a pixel's pairs
// (a block: 2 LP channels) and the block's other 256 / LP lane groups are pixel lanes.  Pixel lane p walks the STRIP / PL consecutive
// pixels [p RUN, (p + 1) RUN) of the strip with the 3x3 window in registers: along a row a pixel loads one new column (three taps,
// issued before the pixel before it is computed) instead of nine.  Out-of-image taps are zeros.  The strip sums are of the fp32 gate
// values before the rounding: a pixel lane's pixels in order, then the pixel lanes in order.
__global__ void __launch_bounds__(256) naf_dw_gate_h_kernel(const _Float16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                            _Float16* __restrict__ y, float* __restrict__ part, int H, int W, int c, int nstrips,
                                                            int lp_shift, int* __restrict__ sat) {
  __shared__ float red[512];   // [pixel lane][2 LP]
  const int LP = 1 << lp_shift, PL = 256 >> lp_shift, RUN = STRIP / PL;
  const int cl = threadIdx.x & (LP - 1), p = threadIdx.x >> lp_shift;
  const int ch = blockIdx.y * 2 * LP + 2 * cl, n = blockIdx.z, strip = blockIdx.x;   // c is even: ch < c covers ch + 1
  const int HW = H * W, C2 = 2 * c;
  float sum0 = 0.f, sum1 = 0.f;
  if (ch < c) {
    float w0[9][2], w1[9][2];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int e = 0; e < 2; ++e) { w0[k][e] = w[k * C2 + ch + e]; w1[k][e] = w[k * C2 + c + ch + e]; }
    const float b00 = b[ch], b01 = b[ch + 1], b10 = b[c + ch], b11 = b[c + ch + 1];
    const _Float16* xn = x + (size_t)n * HW * C2;
    const naf_h2 zero = {(_Float16)0.f, (_Float16)0.f};
    auto ld = [&](int iy, int ix, naf_h2& u, naf_h2& v) {
      u = zero;
      v = zero;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const _Float16* src = xn + ((size_t)iy * W + ix) * C2;
        u = *reinterpret_cast<const naf_h2*>(src + ch);
        v = *reinterpret_cast<const naf_h2*>(src + c + ch);
      }
    };
    int pix = strip * STRIP + p * RUN;
    const int pend = min(pix + RUN, HW);
    int yy = pix / W, xx = pix - yy * W;
    naf_h2 wu[3][3], wv[3][3], nu[3], nv[3];   // the window [row][column] of the two halves, and its next column
    bool fresh = true;
    for (; pix < pend; ++pix) {
      if (fresh) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) ld(yy + dy - 1, xx + dx - 1, wu[dy][dx], wv[dy][dx]);
        fresh = false;
      }
      const bool same_row = xx + 1 < W;
      if (same_row) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) ld(yy + dy - 1, xx + 2, nu[dy], nv[dy]);
      }
      float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          a00 += w0[dy * 3 + dx][0] * (float)wu[dy][dx][0];
          a01 += w0[dy * 3 + dx][1] * (float)wu[dy][dx][1];
          a10 += w1[dy * 3 + dx][0] * (float)wv[dy][dx][0];
          a11 += w1[dy * 3 + dx][1] * (float)wv[dy][dx][1];
        }
      const float g0 = (a00 + b00) * (a10 + b10), g1 = (a01 + b01) * (a11 + b11);
      naf_h2 o;
      o[0] = naf_to_h(g0, sat);
      o[1] = naf_to_h(g1, sat);
      *reinterpret_cast<naf_h2*>(y + ((size_t)n * HW + pix) * c + ch) = o;
      sum0 += g0;
      sum1 += g1;
      if (same_row) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          wu[dy][0] = wu[dy][1]; wu[dy][1] = wu[dy][2]; wu[dy][2] = nu[dy];
          wv[dy][0] = wv[dy][1]; wv[dy][1] = wv[dy][2]; wv[dy][2] = nv[dy];
        }
        ++xx;
      } else {
        xx = 0;
        ++yy;
        fresh = true;
      }
    }
  }
  red[p * 2 * LP + 2 * cl] = sum0;
  red[p * 2 * LP + 2 * cl + 1] = sum1;
  __syncthreads();
  if (p == 0 && ch < c) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      float tot = red[2 * cl + e];
      for (int k = 1; k < PL; ++k) tot += red[k * 2 * LP + 2 * cl + e];
      part[((size_t)n * nstrips + strip) * c + ch + e] = tot;
    }
  }
}

// naf_chansum_kernel on an f16 tensor, two channels per lane
__global__ void __launch_bounds__(256) naf_chansum_h_kernel(const _Float16* __restrict__ x, float* __restrict__ part, int HW, int c, int nstrips) {
  __shared__ float red[4][128];
  const int cl = threadIdx.x & 63, py = threadIdx.x >> 6;
  const int ch = blockIdx.y * 128 + 2 * cl, n = blockIdx.z, strip = blockIdx.x;
  float sum0 = 0.f, sum1 = 0.f;
  if (ch < c)
    for (int q = py; q < STRIP; q += 4) {
      const int pix = strip * STRIP + q;
      if (pix >= HW) break;
      const naf_h2 u = *reinterpret_cast<const naf_h2*>(x + ((size_t)n * HW + pix) * c + ch);
      sum0 += (float)u[0];
      sum1 += (float)u[1];
    }
  red[py][2 * cl] = sum0;
  red[py][2 * cl + 1] = sum1;
  __syncthreads();
  if (py == 0 && ch < c) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
      part[((size_t)n * nstrips + strip) * c + ch + e] = ((red[0][2 * cl + e] + red[1][2 * cl + e]) + red[2][2 * cl + e]) + red[3][2 * cl + e];
  }
}

// naf_enhance_kernel: y = x + (r s + x), eight channels of one pixel per thread (total8 = elements / 8)
__global__ void __launch_bounds__(256) naf_enhance_h_kernel(const _Float16* __restrict__ x, const _Float16* __restrict__ r, const float* __restrict__ s,
                                                            _Float16* __restrict__ y, int HW, int c, size_t total8, int* __restrict__ sat) {
  const size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i8 >= total8) return;
  const size_t i = i8 * 8;
  const int ch = (int)(i % c);
  const size_t n = i / ((size_t)HW * c);
  const naf_h8 xv = *reinterpret_cast<const naf_h8*>(x + i), rv = *reinterpret_cast<const naf_h8*>(r + i);
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(s + n * c + ch), s1 = *reinterpret_cast<const f32x4*>(s + n * c + ch + 4);
  naf_h8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xf = (float)xv[j];
    o[j] = naf_to_h(__fadd_rn(xf, __fadd_rn(__fmul_rn((float)rv[j], j < 4 ? s0[j & 3] : s1[j & 3]), xf)), sat);
  }
  *reinterpret_cast<naf_h8*>(y + i) = o;
}

// fdsr_nafnet_debug_tensor's read-out: the stored values, widened
__global__ void __launch_bounds__(256) naf_widen_h_kernel(const _Float16* __restrict__ src, float* __restrict__ dst, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) dst[i] = (float)src[i];
}
