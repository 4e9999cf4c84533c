// What the transformer families (fdsr_swinir.hip, fdsr_hat.hip, fdsr_transenet.hip) share: the token GEMM with its 3x3 implicit-GEMM gather,
// LayerNorm over channels, the input kernel, the pieces their attention kernels are written from (the 32x32 accumulator's row
// map, the score tile, a window token's pixel and region, the chunk sizes), the host packing of a Linear / Conv2d for the GEMM,
// and the small types of the TABLE / SIZE / RUN walk.  Everything here sits in the anonymous namespace (internal linkage): each
// unit compiles the kernels it launches.  The attention kernels themselves stay in their units: they share source, not code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "fdsr_engine_int.h"

namespace {

using namespace fdsr_int;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 64, BK = 16, NT = 256;
constexpr int AP = BM + 32;   // LDS row pitches: the two k rows an MFMA operand read touches sit 32 banks apart
constexpr int BP = BN + 32;
constexpr int HD = 32;                // head_dim padded to the MFMA tile
constexpr int NUM_FEAT = 64;          // channels of the reconstruction tail
constexpr int LN_MAX_C = 512;         // swin_ln_kernel keeps a row in 8 registers per lane
// the attention kernels that stream their keys (hat_attn_kernel, transenet_attn_kernel)
constexpr int QB = 32;                // queries of one workgroup: a score row pitch of 32 keeps the two k rows of an MFMA operand read 32 banks apart
constexpr int KC = 128;               // keys per staged chunk
constexpr int KP = KC + 32;           // pitch of the [d][key] chunk

// PATCH8: row (b, ty, tx) is the 8 x 8 x Cin patch of an NHWC map, k = (p1 * 8 + p2) * Cin + c (fdsr_transenet.hip)
enum Gather { ROWS = 0, CONV3 = 1, PATCH8 = 2 };
// EPI_EXT and above: epilogues a translation unit adds by defining gemm_epilogue_ext for them
enum Epi { EPI_NONE = 0, EPI_GELU = 1, EPI_LRELU = 2, EPI_RES = 3, EPI_SHUFFLE = 4, EPI_NCHW = 5, EPI_EXT = 6 };

struct GemmArgs {
  const float* x;      // ROWS: [M][K];  CONV3, PATCH8: NHWC [B][H][W][Cin]
  const float* w;      // [Kpad][Npad];  CONV3: k = (ky * 3 + kx) * Cin + ci
  const float* bias;   // [Npad]
  const float* res;    // EPI_RES: [M][N], may be `out`
  float* out;
  int M, N, K, Kpad, Npad;
  int H, W, Cin;       // the feature map the rows are pixels of (CONV3, EPI_SHUFFLE, EPI_NCHW)
  int r;               // EPI_SHUFFLE: the factor
  int Hc, Wc;          // EPI_NCHW: the crop
  float slope;         // EPI_LRELU
  float range, mean[3];   // EPI_NCHW: out = acc / img_range + mean
};

// C/D map of v_mfma_f32_32x32x2_f32: element i of lane (r31 = lane & 31, h = lane >> 5) is column r31 of row (i & 3) + 8 (i >> 2) +
// 4 h of the tile; acc_row adds the tile's first row
__device__ __forceinline__ int acc_row(int row0, int i, int h) { return row0 + (i & 3) + 8 * (i >> 2) + 4 * h; }

// St[j][i] = sum_d k[j][d] q[i][d], one 32 x 32 tile: sK [d][key] and sQ [d][query] in LDS with their pitches, key0 / query0 the
// tile's first key and query column, r31 this lane's column of both; rows of the result are keys, so that stores run along the
// queries
template <int NK, int NQ>
__device__ __forceinline__ f32x16 score_tile(const float (&sK)[NK], int pitchK, int key0, const float (&sQ)[NQ], int pitchQ, int query0, int r31, int h) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int s = 0; s < HD / 2; ++s) {
    const int kr = 2 * s + h;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[kr * pitchK + key0 + r31], sQ[kr * pitchQ + query0 + r31], acc, 0, 0, 0);
  }
  return acc;
}

// Token tok = ty WS + tx of window (wy, wx) of the image rolled by -shift (torch.roll, then window_partition): its pixel
// ((wy WS + ty + shift) mod H, (wx WS + tx + shift) mod W), and its region of the rolled image (three slices per axis: [0, H - WS),
// [H - WS, H - shift), [H - shift, H)) as calculate_mask numbers them; tokens of different regions do not attend to each other
template <int WS>
__device__ __forceinline__ int window_pixel(int wy, int wx, int tok, int shift, int H, int W) {
  static_assert((WS & (WS - 1)) == 0, "the window side is a power of two");
  const int ys = wy * WS + (tok >> __builtin_ctz(WS)), xs = wx * WS + (tok & (WS - 1));
  return ((ys + shift) % H) * W + (xs + shift) % W;
}
template <int WS>
__device__ __forceinline__ int window_region(int wy, int wx, int tok, int shift, int H, int W) {
  const int ys = wy * WS + (tok >> __builtin_ctz(WS)), xs = wx * WS + (tok & (WS - 1));
  const int rh = ys < H - WS ? 0 : ys < H - shift ? 1 : 2, rw = xs < W - WS ? 0 : xs < W - shift ? 1 : 2;
  return shift > 0 ? rh * 3 + rw : 0;
}

// An added epilogue (EPI >= EPI_EXT): the wave's two 32 x 32 accumulators of column `co` (< N), rows acc_row(row0 + mb 32, i, h).
// Declared here, defined by the unit that instantiates it.
template <int EPI, class ARGS>
__device__ void gemm_epilogue_ext(const ARGS& p, const f32x16 (&acc)[2], int row0, int co, int h, float bias);

// One workgroup: BM rows x BN columns; 4 waves in a 2 x 2 grid, each 64 rows x 32 columns (two 32x32 accumulators).  Thread t
// stages row t % BM and k-octet t / BM of every BK chunk (registers prefetch the next chunk while the MFMAs run on this one).
// Rows >= M, out-of-image taps and k >= K read as zero.  VEC: Cin % 4 == 0 (ROWS: K % 4 == 0), so a quad of k is 4 consecutive
// floats of one row / tap, 16-byte aligned.
template <int GATHER, int EPI, bool VEC, class ARGS = GemmArgs>
__global__ void __launch_bounds__(NT) swin_gemm_kernel(ARGS p) {
  __shared__ __attribute__((aligned(16))) float sA[BK * AP];
  __shared__ __attribute__((aligned(16))) float sB[BK * BP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

  const int am = t & (BM - 1), ak = (t >> 7) * 8;
  const int gm = m0 + am;
  const bool mval = gm < p.M;
  int n = 0, oy = 0, ox = 0;
  if (GATHER == CONV3 && mval) {
    const int HW = p.H * p.W;
    n = gm / HW;
    const int r = gm - n * HW;
    oy = r / p.W;
    ox = r - oy * p.W;
  }
  if constexpr (GATHER == PATCH8) {
    if (mval) {
      const int tw = p.W / 8, ntok = (p.H / 8) * tw;
      n = gm / ntok;
      const int r = gm - n * ntok;
      oy = (r / tw) * 8;
      ox = (r - (r / tw) * tw) * 8;
    }
  }
  const int bk = t >> 4, bn = (t & 15) * 4;

  // the address of element k of this thread's row, or null where it reads as zero
  auto src = [&](int k) -> const float* {
    if (!mval || k >= p.K) return nullptr;
    if (GATHER == ROWS) return p.x + (size_t)gm * p.K + k;
    if constexpr (GATHER == PATCH8) {
      const int pp = k / p.Cin, ci = k - pp * p.Cin;
      return p.x + (((size_t)n * p.H + oy + (pp >> 3)) * p.W + ox + (pp & 7)) * p.Cin + ci;
    }
    const int tap = k / p.Cin, ci = k - tap * p.Cin;
    const int ky = tap / 3, kx = tap - ky * 3;
    const int iy = oy + ky - 1, ix = ox + kx - 1;
    if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) return nullptr;
    return p.x + (((size_t)n * p.H + iy) * p.W + ix) * p.Cin + ci;
  };

  float ra[8];
  f32x4 rb;
  auto load = [&](int kc) {
    const int kb = kc * BK;
    if (VEC) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float* s = src(kb + ak + 4 * q);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (s) v = *reinterpret_cast<const f32x4*>(s);
#pragma unroll
        for (int j = 0; j < 4; ++j) ra[4 * q + j] = v[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float* s = src(kb + ak + j);
        ra[j] = s ? *s : 0.f;
      }
    }
    rb = *reinterpret_cast<const f32x4*>(p.w + (size_t)(kb + bk) * p.Npad + n0 + bn);   // rows < Kpad, columns < Npad
  };

  f32x16 acc[2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;

  const int r31 = lane & 31, h = lane >> 5;
  const int nk = p.Kpad / BK;
  load(0);
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();   // the previous chunk's LDS reads are done
#pragma unroll
    for (int j = 0; j < 8; ++j) sA[(ak + j) * AP + am] = ra[j];
    *reinterpret_cast<f32x4*>(sB + bk * BP + bn) = rb;
    __syncthreads();
    if (kc + 1 < nk) load(kc + 1);
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
      // 32x32x2 operands: A[i = lane & 31][k = lane >> 5] (row, k), B[k = lane >> 5][j = lane & 31] (k, column)
      const int kr = 2 * s + h;
      const float bv = sB[kr * BP + wn * 32 + r31];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
        acc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[kr * AP + wm * 64 + mb * 32 + r31], bv, acc[mb], 0, 0, 0);
    }
  }

  // epilogue: column lane & 31, rows acc_row(., i, lane >> 5)
  const int co = n0 + wn * 32 + r31;
  if (co >= p.N) return;
  const float bias = p.bias[co];
  if constexpr (EPI >= EPI_EXT) {
    gemm_epilogue_ext<EPI>(p, acc, m0 + wm * 64, co, h, bias);
    return;
  }
  const int HW = p.H * p.W;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int om = acc_row(m0 + wm * 64 + mb * 32, i, h);
      if (om >= p.M) continue;
      float v = acc[mb][i] + bias;
      if (EPI == EPI_NONE) {
        p.out[(size_t)om * p.N + co] = v;
      } else if (EPI == EPI_GELU) {
        p.out[(size_t)om * p.N + co] = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
      } else if (EPI == EPI_LRELU) {
        p.out[(size_t)om * p.N + co] = v > 0.f ? v : v * p.slope;
      } else if (EPI == EPI_RES) {
        p.out[(size_t)om * p.N + co] = v + p.res[(size_t)om * p.N + co];
      } else {
        const int b = om / HW, pix = om - b * HW;
        const int y = pix / p.W, x = pix - y * p.W;
        if (EPI == EPI_SHUFFLE) {
          // PixelShuffle(r): channel co = c r r + i r + j of pixel (y, x) is channel c of pixel (y r + i, x r + j)
          const int rr = p.r * p.r, c = co / rr, ij = co - c * rr, si = ij / p.r, sj = ij - si * p.r;
          p.out[(((size_t)b * p.H * p.r + (y * p.r + si)) * p.W * p.r + (x * p.r + sj)) * (p.N / rr) + c] = v;
        } else {
          if (y < p.Hc && x < p.Wc) p.out[(((size_t)b * p.N + co) * p.Hc + y) * p.Wc + x] = __fadd_rn(__fdiv_rn(v, p.range), p.mean[co]);
        }
      }
    }
}

// [B][3][H][W] in [0, 1] -> NHWC [B][Hp][Wp][3], (x - mean) * img_range; rows / columns >= H / W mirror (F.pad 'reflect': index
// 2 (H - 1) - y)
__global__ void __launch_bounds__(256) swin_input_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int Hp, int Wp,
                                                         float m0, float m1, float m2, float range, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % 3);
  const size_t pix = i / 3;
  const int px = (int)(pix % Wp), py = (int)((pix / Wp) % Hp);
  const size_t b = pix / ((size_t)Wp * Hp);
  const int sy = py < H ? py : 2 * (H - 1) - py, sx = px < W ? px : 2 * (W - 1) - px;
  const float mean = c == 0 ? m0 : c == 1 ? m1 : m2;
  y[i] = __fmul_rn(__fsub_rn(x[((b * 3 + c) * H + sy) * W + sx], mean), range);
}

// LayerNorm over the C channels of a token: one wave per token, the row in registers; mean and biased variance by a butterfly
// over the wave (every lane ends with the same sums), eps 1e-5
__global__ void __launch_bounds__(256) swin_ln_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ bta,
                                                      float* __restrict__ y, int M, int C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (size_t)row * C;
  float v[LN_MAX_C / 64];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < LN_MAX_C / 64; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < C ? xr[c] : 0.f;
    s += v[j];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < LN_MAX_C / 64; ++j) {
    const int c = lane + 64 * j;
    const float d = c < C ? v[j] - mean : 0.f;
    q += d * d;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = 1.f / sqrtf(q / (float)C + 1e-5f);
  float* yr = y + (size_t)row * C;
#pragma unroll
  for (int j = 0; j < LN_MAX_C / 64; ++j) {
    const int c = lane + 64 * j;
    if (c < C) yr[c] = (v[j] - mean) * rstd * g[c] + bta[c];
  }
}

template <int GATHER, int EPI, class ARGS>
hipError_t launch_swin_gemm(const ARGS& a, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)((a.M + BM - 1) / BM), (unsigned)(a.Npad / BN));
  if (vec) hipLaunchKernelGGL((swin_gemm_kernel<GATHER, EPI, true, ARGS>), grid, dim3(NT), 0, st, a);
  else hipLaunchKernelGGL((swin_gemm_kernel<GATHER, EPI, false, ARGS>), grid, dim3(NT), 0, st, a);
  return hipGetLastError();
}

// A Linear [cout][cin] or a Conv2d [cout][cin][3][3] as the GEMM reads it: the weight [Kpad][Npad] (CONV: k = tap cin + ci; rows
// K..Kpad-1 and columns cout..Npad-1 stay zero), the bias [Npad]
inline int gemm_kpad(bool conv, int cin) { return round_up(conv ? 9 * cin : cin, BK); }
inline int gemm_npad(int cout) { return round_up(cout, BN); }
inline void pack_gemm_tensor(bool conv, bool is_bias, int cin, int cout, const float* host_f32, std::vector<float>& packed) {
  const int Np = gemm_npad(cout);
  if (is_bias) {
    packed.assign((size_t)Np, 0.f);
    std::copy(host_f32, host_f32 + cout, packed.begin());
    return;
  }
  packed.assign((size_t)gemm_kpad(conv, cin) * Np, 0.f);
  if (!conv) {
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci) packed[(size_t)ci * Np + co] = host_f32[(size_t)co * cin + ci];
  } else {
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci)
        for (int tp = 0; tp < 9; ++tp) packed[((size_t)tp * cin + ci) * Np + co] = host_f32[((size_t)co * cin + ci) * 9 + tp];
  }
}

// A tensor in a workspace buffer: [N][H][W][C]
struct T { int buf, H, W, C; };

enum Mode { TABLE, SIZE, RUN };

}  // namespace
