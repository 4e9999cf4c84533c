// What the three NAFNet GEMM kernels share (naf_gemm_kernel, naf_gemm_h3_kernel, naf_gemm_h1_kernel), included by fdsr_nafnet.hip after
// GemmArgs: the implicit-GEMM gather of a staged pixel row, the LN + FiLM / SCA prologue, the epilogue walk over the 32x32 C/D map.
// The k-loops differ (staging layout, buffering, MFMA sequence: DESIGN 15) and stay with their kernels.
#pragma once

typedef _Float16 naf_h8 __attribute__((ext_vector_type(8)));

constexpr int HK = 32;   // k per staged chunk of the f16 kernels: two 32x32x16 steps
constexpr float F16_MAX = 65504.f;

// the output pixel a thread stages: its image, the input position of tap (0, 0), its prologue operands
struct NafRow {
  int n, iy0, ix0;
  bool valid;   // gm < M
  float mean, rstd;
  const float *pm, *pa;
};

template <int PRO>
__device__ __forceinline__ NafRow naf_row(const GemmArgs& p, int gm) {
  const int HWo = p.Hout * p.Wout;
  NafRow row = {0, 0, 0, gm < p.N * HWo, 0.f, 0.f, nullptr, nullptr};
  int oy = 0, ox = 0;
  if (row.valid) {
    row.n = gm / HWo;
    const int r = gm - row.n * HWo;
    oy = r / p.Wout;
    ox = r - oy * p.Wout;
  }
  row.iy0 = oy * p.S - p.P;
  row.ix0 = ox * p.S - p.P;
  if (PRO != PRO_NONE && row.valid) {
    row.pm = p.pmul + (size_t)row.n * p.pstride;
    if (PRO == PRO_LN) {
      row.pa = p.padd + (size_t)row.n * p.pstride;
      row.mean = p.stats[2 * (size_t)gm];
      row.rstd = p.stats[2 * (size_t)gm + 1];
    }
  }
  return row;
}

// k = (ky * KW + kx) * Cin + ci of the row's pixel: the element offset of x[n][iy][ix][ci]; false where the tap reads as zero
// (outside the image, k >= K, a pixel past M)
__device__ __forceinline__ bool naf_tap(const GemmArgs& p, const NafRow& row, int k, int& ci, size_t& off) {
  if (!(row.valid && k < p.K)) return false;
  const int tap = k / p.Cin;
  ci = k - tap * p.Cin;
  const int ky = tap / p.KW, kx = tap - ky * p.KW;
  const int iy = row.iy0 + ky, ix = row.ix0 + kx;
  if (!(iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win)) return false;
  off = (((size_t)row.n * p.Hin + iy) * p.Win + ix) * p.Cin + ci;
  return true;
}

// the prologue on one value: LN + FiLM, or the SCA multiply
template <int PRO>
__device__ __forceinline__ float naf_pro(float v, float mean, float rstd, float m, float a) {
  return PRO == PRO_LN ? (v - mean) * rstd * m + a : PRO == PRO_MUL ? v * m : v;
}

// the non-VEC gather (intro: Cin % 8 != 0, fp32 xin, no prologue): NJ consecutive k, each with a tap of its own
template <int NJ>
__device__ __forceinline__ void naf_gather_scalar(const GemmArgs& p, const NafRow& row, int k0, float* dst) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    int ci;
    size_t off;
    dst[j] = naf_tap(p, row, k0 + j, ci, off) ? p.x[off] : 0.f;
  }
}

// the VEC gather of an fp32 input: the octet at k lies inside one tap (Cin % 8 == 0); prologue applied
template <int PRO>
__device__ __forceinline__ void naf_gather_octet(const GemmArgs& p, const NafRow& row, int k, float* dst) {
  f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
  int ci;
  size_t off;
  if (naf_tap(p, row, k, ci, off)) {
    const f32x4* src = reinterpret_cast<const f32x4*>(p.x + off);
    v0 = src[0];
    v1 = src[1];
    if (PRO != PRO_NONE) {
      const f32x4 m0v = *reinterpret_cast<const f32x4*>(row.pm + ci), m1v = *reinterpret_cast<const f32x4*>(row.pm + ci + 4);
      f32x4 a0v = {0.f, 0.f, 0.f, 0.f}, a1v = a0v;
      if (PRO == PRO_LN) {
        a0v = *reinterpret_cast<const f32x4*>(row.pa + ci);
        a1v = *reinterpret_cast<const f32x4*>(row.pa + ci + 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v0[j] = naf_pro<PRO>(v0[j], row.mean, row.rstd, m0v[j], a0v[j]);
        v1[j] = naf_pro<PRO>(v1[j], row.mean, row.rstd, m1v[j], a1v[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { dst[j] = v0[j]; dst[4 + j] = v1[j]; }
}

__device__ __forceinline__ void naf_zero(f32x16 (&acc)[2]) {
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
}

// The f16 kernels' weight fragments [column tile][chunk][nb][s][plane][lane] x 16 B (split_weights): element j of lane l is
// w[k = 32 chunk + 16 s + 8 (l >> 5) + j][column = 64 tile + 32 nb + (l & 31)] (the 32x32x16 B operand map).  The hi plane of
// fragment (kc, nb, s) for this lane; the lo plane is 64 further.
__device__ __forceinline__ const uint4* naf_bfrag(const GemmArgs& p, int nk, int lane, int kc, int nb, int s) {
  return p.wq + ((size_t)blockIdx.y * nk * 8) * 64 + lane + ((size_t)kc * 8 + nb * 4 + s * 2) * 64;
}

// 32x32x16 A operand: A[i = lane & 31][k = 8 (lane >> 5) + j] (pixel, k), from LDS rows of `pitch` bytes per pixel
__device__ __forceinline__ int naf_aoff(int lane, int wave, int pitch) { return (wave * 32 + (lane & 31)) * pitch + 16 * (lane >> 5); }

// The epilogue of a wave's two 32x32 accumulators (pixels x packed columns [co0, co0 + 64) of the tile at pixel m0): bias, then the
// gate / ReLU / residual / PixelShuffle form GemmArgs::epi names.  The policy E says what differs between the kernels:
//   E::SCALE, e.winv()       the accumulator is un-scaled by winv before the bias (not `* 1`: the fp32 kernel keeps acc + bias)
//   e.res(oi)                the residual at element oi of the output
//   e.put(oi, row, col, v)   a finished value: element oi of the output, (pixel row, column) of the tile
//   e.pair(om, cg, u0, u1)   EPI_GATE: the pair before the gate
template <class E>
__device__ __forceinline__ void naf_epilogue(const GemmArgs& p, const f32x16 (&acc)[2], int m0, int co0, int lane, int wave, const E& e) {
  const int HWo = p.Hout * p.Wout;
  const int M = p.N * HWo;
  const int r31 = lane & 31;
  auto biased = [&](float a, float b) {
    if constexpr (E::SCALE) return a * e.winv() + b;
    else return a + b;
  };
  // C/D map: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (pixel)
  auto tile_row = [&](int i) { return wave * 32 + 4 * (lane >> 5) + (i & 3) + 8 * (i >> 2); };
  if (p.epi == EPI_GATE) {
    // packed columns [64 q, 64 q + 32) are channels 32 q + r of the first half, [64 q + 32, 64 q + 64) the same channels of the second
    const int cg = blockIdx.y * 32 + r31;
    if (cg >= (p.Cout >> 1)) return;
    const float b0 = p.bias[co0 + r31], b1 = p.bias[co0 + 32 + r31];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = tile_row(i), om = m0 + row;
      if (om >= M) continue;
      const float u0 = biased(acc[0][i], b0), u1 = biased(acc[1][i], b1);
      e.put((size_t)om * p.ostride + cg, row, r31, u0 * u1);
      e.pair(om, cg, u0, u1);
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
      const int row = tile_row(i), om = m0 + row;
      if (om >= M) continue;
      const float v = biased(acc[nb][i], bias);
      if (p.epi == EPI_PSHUF) {
        // PixelShuffle(2): out[n][c][2y + dy][2x + dx] = in[n][4c + 2dy + dx][y][x], then + enc_skip
        const int pn = om / HWo, r = om - pn * HWo;
        const int y = r / p.Wout, x = r - y * p.Wout;
        const int c = co >> 2, dy = (co >> 1) & 1, dx = co & 1;
        const size_t oi = (((size_t)pn * 2 * p.Hout + 2 * y + dy) * 2 * p.Wout + 2 * x + dx) * p.ostride + c;
        e.put(oi, row, nb * 32 + r31, v + e.res(oi));
      } else {
        const size_t oi = (size_t)om * p.ostride + co;
        e.put(oi, row, nb * 32 + r31, p.epi == EPI_RELU ? fmaxf(v, 0.f) : p.epi == EPI_RES ? e.res(oi) + v * ev : v);
      }
    }
  }
}

// fp32 output in global memory: naf_gemm_kernel (SCALE false) and naf_gemm_h3_kernel (SCALE true).  out2 is training's: fp32 here
// (the host refuses it for f16x3); under f16 training storage the f16 kernel's policy stores it (fdsr_nafnet_h1.h).
template <bool SCALE_>
struct NafEpiF32 {
  static constexpr bool SCALE = SCALE_;
  const GemmArgs& p;
  __device__ __forceinline__ float winv() const { return p.winv; }
  __device__ __forceinline__ float res(size_t oi) const { return p.res[oi]; }
  __device__ __forceinline__ void put(size_t oi, int, int, float v) const { p.out[oi] = v; }
  __device__ __forceinline__ void pair(int om, int cg, float u0, float u1) const {
    if constexpr (!SCALE)
      if (p.out2) {
        p.out2[(size_t)om * p.Cout + cg] = u0;
        p.out2[(size_t)om * p.Cout + (p.Cout >> 1) + cg] = u1;
      }
  }
};
