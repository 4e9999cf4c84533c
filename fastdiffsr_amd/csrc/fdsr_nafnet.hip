// EDiffSR on gfx950: ConditionalNAFNet (EDiffSR/codes/config/sisr/models/modules/DenoisingNAFNet_arch.py, module_util.py) and the
// IR-SDE reverse process (utils/sde_utils.py: IRSDE.reverse_sde / reverse_ode), fp32 NHWC activations.
//
//   NAFBlock(inp, t):  shift_att, scale_att, shift_ffn, scale_ffn = Linear(SimpleGate(t)).chunk(4)
//     x = conv1(LayerNorm1(inp) (scale_att + 1) + shift_att)        1x1, c -> 2c     LN + FiLM in the GEMM's prologue
//     x = SimpleGate(conv2(x))                                      depthwise 3x3    one kernel, with the pool's partial sums
//     x = conv3(x * sca(x));  y = inp + x beta                      1x1, c -> c      SCA scale in the prologue, residual in the epilogue
//     x = SimpleGate(conv4(LayerNorm2(y) (scale_ffn + 1) + shift_ffn))   1x1, c -> 2c   gate in the epilogue (column j with j + c)
//     out = y + conv5(x) gamma                                      1x1, c -> c
//
// Every convolution that is a GEMM (1x1, the 2x2 stride-2 downs, the dense 3x3 of intro / enhance / ending) runs on one implicit-GEMM
// kernel on v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered chain per output, no split-K, no atomics.  Pools are per-strip partial
// sums added in a fixed order.  Every output element has one summation order that depends neither on B nor on the image's place
// in the batch: reruns are bitwise identical.  LayerNorm: over channels per pixel, biased variance (two passes), eps 1e-5.
// Two opt-in sampling modes pick other kernels in the same walk: FDSR_PREC_F16X3 (fdsr_nafnet_h3.h: the GEMMs on an fp32-grade f16 split)
// and FDSR_NAF_STORE_F16 (fdsr_nafnet_h1.h: f16 activations in memory, one f16 MFMA per product).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "fdsr_act_io.h"
#include "fdsr_engine_int.h"
#include "fdsr_philox.h"

using namespace fdsr_int;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 64, BK = 16, NT = 256;
constexpr int AP = BM + 32;   // LDS row pitches: the two k rows an MFMA operand read touches sit 32 banks apart
constexpr int BP = BN + 32;
constexpr int STRIP = 256;    // pixels per partial sum of a global average pool
constexpr float LN_EPS = 1e-5f;

enum { PRO_NONE = 0, PRO_MUL = 1, PRO_LN = 2 };
enum { EPI_BIAS = 0, EPI_RELU = 1, EPI_GATE = 2, EPI_RES = 3, EPI_PSHUF = 4 };

struct GemmArgs {
  const float* x;      // fp32 NHWC input [N][Hin][Win][Cin]
  const float* w;      // [Kpad][CoutPad], k = (ky * KW + kx) * Cin + ci
  const float* bias;   // [CoutPad] (zeros for a bias-free conv)
  float* out;
  float* out2;         // EPI_GATE, training: the pair before the gate, [M][Cout] in channel order (or null)
  const float* stats;  // PRO_LN: [M][2] (mean, rstd) per pixel
  const float* pmul;   // PRO_MUL / PRO_LN: per-image vector over k, a = a * pmul[k]      (image n at pmul + n * pstride)
  const float* padd;   // PRO_LN: a = (a - mean) rstd pmul[k] + padd[k]
  const float* res;    // EPI_RES: out = res + v evec[co];  EPI_PSHUF: out = v + res (the encoder skip)
  const float* evec;
  int N, Hin, Win, Cin, Hout, Wout, Cout, KW, S, P, K, Kpad, CoutPad, ostride, pstride, epi;
  // FDSR_PREC_F16X3 (naf_gemm_h3_kernel): the split weight fragments, 2^-e of their scale, the sticky range flag
  const uint4* wq;
  float winv;
  int* sat;
  // FDSR_NAF_STORE_F16 (naf_gemm_h1_kernel): x (but for intro's fp32 xin), res and out are f16; o32: out is fp32 (ending's eps)
  int o32;
  // training under f16 storage (fdsr_nafnet_set_train_storage): 2^-e from the device table the weight rebuild writes (null: winv);
  // out2 is f16 there
  const float* winvp;
};

#include "fdsr_nafnet_gemm.h"

// One workgroup: BM output pixels x BN packed output columns; 4 waves, each 32 pixels x 64 columns (two 32x32 accumulators, so the
// two halves of a gated pair sit in one lane).  Thread t stages pixel t % BM and k-octet t / BM of every BK chunk; registers prefetch
// the next chunk while the MFMAs run on this one.  Out-of-image taps and k >= K read as zero.  VEC: Cin % 8 == 0 (all but intro).
// PRO != PRO_NONE is used with 1x1 convolutions only (k == input channel).
template <int PRO, bool VEC>
__global__ void __launch_bounds__(NT) naf_gemm_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) float sA[BK * AP];
  __shared__ __attribute__((aligned(16))) float sB[BK * BP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.x * BM, co0 = blockIdx.y * BN;

  const int am = t & (BM - 1), ak = (t >> 7) * 8;
  const NafRow row = naf_row<PRO>(p, m0 + am);
  const int bk = t >> 4, bn = (t & 15) * 4;

  float ra[8];
  f32x4 rb;
  auto load = [&](int kc) {
    const int kb = kc * BK;
    if (VEC) naf_gather_octet<PRO>(p, row, kb + ak, ra);
    else naf_gather_scalar<8>(p, row, kb + ak, ra);
    rb = *reinterpret_cast<const f32x4*>(p.w + (size_t)(kb + bk) * p.CoutPad + co0 + bn);   // rows < Kpad, columns < CoutPad
  };

  f32x16 acc[2];
  naf_zero(acc);

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
      // 32x32x2 operands: A[i = lane & 31][k = lane >> 5] (pixel, k), B[k = lane >> 5][j = lane & 31] (k, column)
      const int kr = 2 * s + h;
      const float av = sA[kr * AP + wave * 32 + r31];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, sB[kr * BP + nb * 32 + r31], acc[nb], 0, 0, 0);
    }
  }
  naf_epilogue(p, acc, m0, co0, lane, wave, NafEpiF32<false>{p});
}

#include "fdsr_nafnet_h3.h"
#include "fdsr_nafnet_h1.h"

// LayerNorm statistics: (mean, 1 / sqrt(var + eps)) per pixel over C channels, biased variance, two passes.  16 lanes per pixel,
// a butterfly of commutative adds: every lane ends with the same bits.
__global__ void __launch_bounds__(256) naf_ln_stats_kernel(const float* __restrict__ x, float* __restrict__ stats, int M, int C) {
  const int sub = threadIdx.x & 15;
  const int pix = blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool ok = pix < M;
  const float* row = x + (size_t)(ok ? pix : 0) * C;
  float s = 0.f;
  for (int c = sub * 4; c < C; c += 64) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
#pragma unroll
  for (int o = 8; o; o >>= 1) s += __shfl_xor(s, o, 16);
  const float mean = s / (float)C;
  float q = 0.f;
  for (int c = sub * 4; c < C; c += 64) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
    const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
#pragma unroll
  for (int o = 8; o; o >>= 1) q += __shfl_xor(q, o, 16);
  if (ok && sub == 0) {
    stats[2 * (size_t)pix] = mean;
    stats[2 * (size_t)pix + 1] = 1.f / sqrtf(q / (float)C + LN_EPS);
  }
}

// conv2 (depthwise 3x3, padding 1, bias) + SimpleGate: y[.., ch] = dw(x)[ch] * dw(x)[ch + c], and the strip's channel sums of y for
// SCA's global average (part[n][strip][ch]: pixels of the strip in order per pixel lane, then the four lanes in order).
__global__ void __launch_bounds__(256) naf_dw_gate_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                          float* __restrict__ y, float* __restrict__ part, int H, int W, int c, int nstrips) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, py = threadIdx.x >> 6;
  const int ch = blockIdx.y * 64 + cl, n = blockIdx.z, strip = blockIdx.x;
  const int HW = H * W, C2 = 2 * c;
  float sum = 0.f;
  if (ch < c) {
    float w0[9], w1[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { w0[k] = w[k * C2 + ch]; w1[k] = w[k * C2 + c + ch]; }
    const float b0 = b[ch], b1 = b[c + ch];
    const float* xn = x + (size_t)n * HW * C2;
    for (int q = py; q < STRIP; q += 4) {
      const int pix = strip * STRIP + q;
      if (pix >= HW) break;
      const int yy = pix / W, xx = pix - yy * W;
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int iy = yy + dy - 1, ix = xx + dx - 1;
          if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
          const float* src = xn + ((size_t)iy * W + ix) * C2;
          a0 += w0[dy * 3 + dx] * src[ch];
          a1 += w1[dy * 3 + dx] * src[c + ch];
        }
      const float g = (a0 + b0) * (a1 + b1);
      y[((size_t)n * HW + pix) * c + ch] = g;
      sum += g;
    }
  }
  red[py][cl] = sum;
  __syncthreads();
  if (py == 0 && ch < c) part[((size_t)n * nstrips + strip) * c + ch] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// the same strip sums for a tensor that exists already (RCAB's ChannelAttention pool)
__global__ void __launch_bounds__(256) naf_chansum_kernel(const float* __restrict__ x, float* __restrict__ part, int HW, int c, int nstrips) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, py = threadIdx.x >> 6;
  const int ch = blockIdx.y * 64 + cl, n = blockIdx.z, strip = blockIdx.x;
  float sum = 0.f;
  if (ch < c)
    for (int q = py; q < STRIP; q += 4) {
      const int pix = strip * STRIP + q;
      if (pix >= HW) break;
      sum += x[((size_t)n * HW + pix) * c + ch];
    }
  red[py][cl] = sum;
  __syncthreads();
  if (py == 0 && ch < c) part[((size_t)n * nstrips + strip) * c + ch] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// pooled[ci] = (the strips' sums: G interleaved groups in order, then the groups in order) / HW, into LDS
__device__ __forceinline__ void pooled_to_lds(const float* __restrict__ part, int n, int nstrips, int HW, int c, float* pooled, float* tmp) {
  const int cw = c < 256 ? c : 256, G = 256 / cw;
  const int g = threadIdx.x / cw, cl = threadIdx.x - g * cw;
  for (int c0 = 0; c0 < c; c0 += cw) {
    const int ci = c0 + cl;
    float s = 0.f;
    if (g < G && ci < c)
      for (int st = g; st < nstrips; st += G) s += part[((size_t)n * nstrips + st) * c + ci];
    if (g < G) tmp[g * cw + cl] = s;
    __syncthreads();
    if (g == 0 && ci < c) {
      float tot = tmp[cl];
      for (int k = 1; k < G; ++k) tot += tmp[k * cw + cl];
      pooled[ci] = tot / (float)HW;
    }
    __syncthreads();
  }
}

// SCA: s[n][co] = b[co] + sum_ci W[co][ci] pooled[n][ci].  Block: 16 output channels of one image (4 per wave).
__global__ void __launch_bounds__(256) naf_sca_kernel(const float* __restrict__ part, int nstrips, int HW, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ out, int c) {
  extern __shared__ float lds[];
  float* pooled = lds;
  float* tmp = lds + c;
  const int n = blockIdx.y;
  pooled_to_lds(part, n, nstrips, HW, c, pooled, tmp);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = 0; j < 4; ++j) {
    const int co = blockIdx.x * 16 + wave * 4 + j;   // wave-uniform
    if (co >= c) break;
    float a = 0.f;
    for (int ci = lane; ci < c; ci += 64) a += w[(size_t)co * c + ci] * pooled[ci];
#pragma unroll
    for (int o = 32; o; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) out[(size_t)n * c + co] = a + b[co];
  }
}

// RCAB's ChannelAttention: pooled -> conv1x1 (c -> cs) -> ReLU -> conv1x1 (cs -> c) -> sigmoid.  One block per image.
__global__ void __launch_bounds__(256) naf_ca_kernel(const float* __restrict__ part, int nstrips, int HW, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                     float* __restrict__ out, int c, int cs) {
  extern __shared__ float lds[];
  float* pooled = lds;
  float* tmp = lds + c;
  float* hid = tmp + 256;
  const int n = blockIdx.x;
  pooled_to_lds(part, n, nstrips, HW, c, pooled, tmp);
  for (int j = threadIdx.x; j < cs; j += 256) {
    float a = b1[j];
    for (int ci = 0; ci < c; ++ci) a += w1[(size_t)j * c + ci] * pooled[ci];
    hid[j] = fmaxf(a, 0.f);
  }
  __syncthreads();
  for (int co = threadIdx.x; co < c; co += 256) {
    float a = b2[co];
    for (int j = 0; j < cs; ++j) a += w2[(size_t)co * cs + j] * hid[j];
    out[(size_t)n * c + co] = 1.f / (1.f + expf(-a));
  }
}

// x = x + enhance(x), enhance(x) = rcab(x) + x, rcab(x) = r * s: y = x + (r s + x)
__global__ void __launch_bounds__(256) naf_enhance_kernel(const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ s,
                                                          float* __restrict__ y, int HW, int c, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % c);
  const size_t n = i / ((size_t)HW * c);
  y[i] = __fadd_rn(x[i], __fadd_rn(__fmul_rn(r[i], s[n * c + ch]), x[i]));
}

// cat[x - cond, cond], zero-padded right / bottom to Hp x Wp, NCHW -> NHWC [N][Hp][Wp][6]
__global__ void __launch_bounds__(256) naf_prep_kernel(const float* __restrict__ x, const float* __restrict__ cond, float* __restrict__ xin, int H,
                                                       int W, int Hp, int Wp, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int px = (int)(i % Wp), py = (int)((i / Wp) % Hp);
  const size_t n = i / ((size_t)Wp * Hp);
  const bool in = py < H && px < W;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float a = 0.f, m = 0.f;
    if (in) {
      const size_t si = ((n * 3 + c) * H + py) * W + px;
      m = cond[si];
      a = __fsub_rn(x[si], m);
    }
    xin[i * 6 + c] = a;
    xin[i * 6 + 3 + c] = m;
  }
}

struct StepTables { const float *theta, *sigma, *sbar; float dt, sqrt_dt; int T; };

// The tail of a forward: crop the padded NHWC prediction.  mode 0: out = eps (NCHW).  mode 1 / 2: one reverse SDE / ODE step on
// x (in place, NCHW) for step k = ctl[0], t = T - k; rounded operations in the reference's order.
__global__ void __launch_bounds__(256) naf_tail_kernel(const float* __restrict__ eps, float* __restrict__ x, const float* __restrict__ cond,
                                                       const float* __restrict__ noise, float* __restrict__ traj, const int* __restrict__ ctl,
                                                       StepTables tb, unsigned long long seed, long long first_image,
                                                       const int* __restrict__ tiles, int scene_w, int mode, int H, int W, int Hp, int Wp,
                                                       size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // (n, y, x) of the cropped image
  if (i >= total) return;
  const int px = (int)(i % W), py = (int)((i / W) % H);
  const size_t n = i / ((size_t)W * H);
  const float* e = eps + ((n * Hp + py) * Wp + px) * 3;
  const size_t HW = (size_t)H * W, base = n * 3 * HW + (size_t)py * W + px;
  if (mode == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[base + c * HW] = e[c];
    return;
  }
  const int k = ctl[0], t = tb.T - k;
  const float theta = tb.theta[t], sigma = tb.sigma[t], sbar = tb.sbar[t];
  const float s2 = __fmul_rn(sigma, sigma);
  float z[3] = {0.f, 0.f, 0.f};
  const size_t plane = (size_t)k * (total * 3);
  if (mode == 1) {
    if (noise) {
#pragma unroll
      for (int c = 0; c < 3; ++c) z[c] = noise[plane + base + c * HW];
    } else {
      const unsigned long long rng[2] = {seed, 0ull};
      // the pixel's position among the images of the whole run, or in the scene the images are tiles of (fdsr_nafnet_set_noise_tiles)
      fdsr::randn3(rng, k, tiles ? fdsr::tile_counter(tiles, scene_w, W, n, (size_t)py * W + px) : (size_t)first_image * HW + i, z);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float xv = x[base + c * HW], mu = cond[base + c * HW];
    const float score = __fdiv_rn(-e[c], sbar);
    const float a = __fmul_rn(theta, __fsub_rn(mu, xv));
    float v;
    if (mode == 1) {
      const float drift = __fmul_rn(__fsub_rn(a, __fmul_rn(s2, score)), tb.dt);
      v = __fsub_rn(__fsub_rn(xv, drift), __fmul_rn(sigma, __fmul_rn(z[c], tb.sqrt_dt)));
    } else {
      const float drift = __fmul_rn(__fsub_rn(a, __fmul_rn(__fmul_rn(0.5f, s2), score)), tb.dt);
      v = __fsub_rn(xv, drift);
    }
    x[base + c * HW] = v;
    if (traj) traj[plane + base + c * HW] = v;
  }
}

__global__ void naf_row_copy_kernel(const float* __restrict__ table, float* __restrict__ row, const int* __restrict__ ctl, int T, int R) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < R) row[i] = table[(size_t)(T - ctl[0]) * R + i];
}

__global__ void naf_advance_kernel(int* ctl) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ctl[0] += 1;
}

__global__ void naf_iota_kernel(float* t, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) t[i] = (float)i;
}

__global__ void __launch_bounds__(256) naf_randn_kernel(float* __restrict__ dst, int HW, int plane, unsigned long long seed, size_t pix0, size_t total,
                                                        const int* __restrict__ tiles, int scene_w, int W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const unsigned long long rng[2] = {seed, 0ull};
  const size_t n = i / HW, pix = i % HW;
  float z[3];
  fdsr::randn3(rng, plane, tiles ? fdsr::tile_counter(tiles, scene_w, W, n, pix) : i + pix0, z);
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[(n * 3 + c) * HW + pix] = z[c];
}

// time_mlp and the blocks' SimpleGate: emb = [sin(t f), cos(t f)] (fp32, as SinusoidalPosEmb on an fp32 time) -> Linear(w, 8w) ->
// SimpleGate -> Linear(4w, 4w) -> SimpleGate (the first op of every NAFBlock.mlp): tg[b][2w].  One block per time value.
__global__ void __launch_bounds__(256) naf_time_kernel(const float* __restrict__ time, const float* __restrict__ freq, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                       float* __restrict__ tg, int wd) {
  extern __shared__ float lds[];
  float* emb = lds;            // [wd]
  float* h1 = emb + wd;        // [8 wd]
  float* g1 = h1 + 8 * wd;     // [4 wd]
  float* h2 = g1 + 4 * wd;     // [4 wd]
  const int b = blockIdx.x, half = wd / 2;
  const float tv = time[b];
  for (int j = threadIdx.x; j < wd; j += 256) {
    const float a = __fmul_rn(tv, freq[j < half ? j : j - half]);
    emb[j] = j < half ? sinf(a) : cosf(a);
  }
  __syncthreads();
  for (int r = threadIdx.x; r < 8 * wd; r += 256) {
    float a = 0.f;
    for (int j = 0; j < wd; ++j) a += w1[(size_t)r * wd + j] * emb[j];
    h1[r] = a + b1[r];
  }
  __syncthreads();
  for (int r = threadIdx.x; r < 4 * wd; r += 256) g1[r] = h1[r] * h1[r + 4 * wd];
  __syncthreads();
  for (int r = threadIdx.x; r < 4 * wd; r += 256) {
    float a = 0.f;
    for (int j = 0; j < 4 * wd; ++j) a += w2[(size_t)r * 4 * wd + j] * g1[j];
    h2[r] = a + b2[r];
  }
  __syncthreads();
  for (int r = threadIdx.x; r < 2 * wd; r += 256) tg[(size_t)b * 2 * wd + r] = h2[r] * h2[r + 2 * wd];
}

// every block's Linear(2w, 4c) at once: rows[b][r] = ((W[r] . tg[b] + bias[r]) + add[r]) * mul[r]; (add, mul) = (1, g) on the scale
// rows -- the LayerNorm gain folded into (scale + 1) -- and (0, 1) on the shift rows.  wT is [2w][R].
__global__ void __launch_bounds__(256) naf_rows_kernel(const float* __restrict__ tg, const float* __restrict__ wT, const float* __restrict__ bias,
                                                       const float* __restrict__ add, const float* __restrict__ mul, float* __restrict__ rows, int K,
                                                       int R) {
  const int r = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (r >= R) return;
  float a = 0.f;
  for (int j = 0; j < K; ++j) a += wT[(size_t)j * R + r] * tg[(size_t)b * K + j];
  rows[(size_t)b * R + r] = ((a + bias[r]) + add[r]) * mul[r];
}

// F.interpolate(scale_factor = s, mode = 'bicubic', align_corners = False): A = -0.75, src = (d + 0.5) / s - 0.5, taps clamped.
__global__ void __launch_bounds__(256) naf_upscale_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int s, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int Wo = W * s, Ho = H * s;
  const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
  const size_t nc = i / ((size_t)Wo * Ho);
  const double sc = 1.0 / (double)s, A = -0.75;
  auto coef = [&](int o, int& i0, double* cf) {
    const double r = sc * (o + 0.5) - 0.5, f = floor(r), t = r - f;
    i0 = (int)f;
    const double x0 = t + 1.0, x3 = (1.0 - t) + 1.0, u = 1.0 - t;
    cf[0] = ((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A;
    cf[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
    cf[2] = ((A + 2.0) * u - (A + 3.0)) * u * u + 1.0;
    cf[3] = ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A;
  };
  int ix, iy;
  double cx[4], cy[4];
  coef(ox, ix, cx);
  coef(oy, iy, cy);
  const float* p = src + nc * (size_t)H * W;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = min(max(iy - 1 + k, 0), H - 1);
    double row = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) row += (double)p[(size_t)yy * W + min(max(ix - 1 + j, 0), W - 1)] * cx[j];
    acc += row * cy[k];
  }
  dst[i] = (float)acc;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct WT {
  std::string key;
  std::vector<int64_t> shape;
  std::vector<float> host;
  bool loaded = false;
};

struct GemmL {
  int w = -1, b = -1;   // weight-table indices (b < 0: no bias)
  int cin = 0, cout = 0, ks = 1, s = 1, p = 0;
  bool gate = false;
  size_t woff = 0, boff = 0;   // float offsets into the device arena
  size_t hoff = 0;             // f16x3 (the forward GEMMs; build_schema): the split form's first 16-byte fragment
  int hidx = 0;                //        its entry in the device table of scales (d_hinv)
  float hinv = 1.f;            //        2^-e of the split form's scale (split_weights)
  int K32() const { return round_up(K(), HK); }
  size_t hfrags() const { return (size_t)(CoutPad() / BN) * (K32() / HK) * 8 * 64; }
  int K() const { return ks * ks * cin; }
  int Kpad() const { return round_up(K(), BK); }
  int CoutPad() const { return gate ? 2 * round_up(cout / 2, 32) : round_up(cout, BN); }
};

struct BlockL {
  std::string name;
  int c = 0;
  int beta = -1, gamma = -1, mlpw = -1, mlpb = -1, dww = -1, dwb = -1, scaw = -1, scab = -1, g1 = -1, g2 = -1;
  int conv1 = -1, conv3 = -1, conv4 = -1, conv5 = -1;   // GemmL indices
  size_t off_beta = 0, off_gamma = 0, off_dww = 0, off_dwb = 0, off_scaw = 0, off_scab = 0;
  int row_off = 0;   // first of its 4c rows in the time-row table
};

struct Plan {
  int N, H, W, Hp, Wp;
  size_t xin, A, B, T1, T2, stats, part, sca, ca, tg, trow, eps, bytes;
  std::vector<size_t> skip;
};

}  // namespace

struct fdsr_nafnet_obj {
  fdsr_nafnet_config cfg{};
  int L = 0, wd = 0, R = 0;
  std::vector<WT> wts;
  std::map<std::string, int> key2w;
  std::vector<GemmL> gemms, tgemms;   // tgemms[i]: the input gradient of gemms[i] as a convolution of its own
  std::vector<size_t> poff;           // tensor i's first element in the flat master / gradient / optimizer-state buffers
  size_t P = 0, off_zero = 0;
  std::vector<BlockL> blocks;
  std::vector<std::vector<int>> enc, dec;
  std::vector<int> mid, ups, downs;   // ups / downs: GemmL indices
  int g_intro = -1, g_rcab0 = -1, g_rcab2 = -1, g_ending = -1;
  int t1w = -1, t1b = -1, t2w = -1, t2b = -1, ca1w = -1, ca1b = -1, ca2w = -1, ca2b = -1;
  size_t off_freq = 0, off_t1w = 0, off_t1b = 0, off_t2w = 0, off_t2b = 0, off_ca1w = 0, off_ca1b = 0, off_ca2w = 0, off_ca2b = 0;
  size_t off_rowsw = 0, off_rowsb = 0, off_rowsadd = 0, off_rowsmul = 0;
  size_t arena_floats = 0;
  float* d_arena = nullptr;
  bool dirty = true;
  // FDSR_PREC_F16X3: hi / lo planes of the forward GEMMs' weights (built by finalize in that mode) and the range flag
  int prec = FDSR_PREC_F32;
  int store = FDSR_NAF_STORE_F32;   // FDSR_NAF_STORE_F16: f16 activations, the hi planes of d_wq, the same flag (fdsr_nafnet_h1.h)
  int train_store = FDSR_NAF_STORE_F32;   // training's own storage setting.  What the three make of a call: mode_of
  size_t hfrags = 0;
  uint4* d_wq = nullptr;
  float* d_hinv = nullptr;   // [gemms]: 2^-e of every split form, as split_weights / naf_wq_scale_kernel left it
  void* d_hdesc = nullptr;   // [gemms] WqDesc: where the device rebuild of d_wq finds each GEMM (fdsr_nafnet_train.h)
  int *d_sat = nullptr, *h_sat = nullptr;
  // training (fdsr_nafnet_train.h): flat fp32 buffers in the reference's layout, tensors in state_dict order
  float *d_master = nullptr, *d_grad = nullptr, *d_m = nullptr, *d_v = nullptr, *d_cum = nullptr;
  int *d_map = nullptr, *d_rowmap = nullptr;
  bool master_valid = false;   // d_master holds the weights the arena was packed from
  bool host_stale = false;     // an optimizer step moved the weights on: the host copies are behind d_master
  long long opt_step = 0;
  int cum_T = 0;
  // the autograd bridge (fdsr_nafnet_forward_train / _backward): the ticket of the activations a training workspace holds (0: none),
  // the call they belong to, and what made the last ticket stale
  struct { long long next = 0, live = 0; int N = 0, H = 0, W = 0; const void* ws = nullptr; const char* killer = "no fdsr_nafnet_forward_train yet"; } ticket;
  // IR-SDE
  int T = 0;
  std::vector<float> thetas, sigmas, sbars;
  float dt = 0.f;
  float* d_sde = nullptr;        // [3][T + 1]
  float* d_rowtable = nullptr;   // [T + 1][R]: the blocks' time rows of t = 0 .. T
  bool table_valid = false;
  float* d_cur_row = nullptr;    // [R]: the current step's rows
  int* d_ctl = nullptr;          // step counter
  // one cached step graph
  struct { const void *cond = nullptr, *noise = nullptr, *out = nullptr, *traj = nullptr, *ws = nullptr; int N = 0, H = 0, W = 0, flags = 0;
           unsigned long long seed = 0; long long first = 0; const void* tiles = nullptr; int scene_w = 0; hipGraphExec_t exec = nullptr; } graph;
  NoiseTileTable noise_tiles;    // fdsr_nafnet_set_noise_tiles: the caller's device table of tile origins, or none
};

namespace {

// the activations fdsr_nafnet_forward_train kept are overwritten, or no longer those of the weights: its ticket is stale from here on
void kill_ticket(fdsr_nafnet n, const char* by) {
  if (n->ticket.live) n->ticket.killer = by;
  n->ticket.live = 0;
}

void drop_graph(fdsr_nafnet n) {
  if (n->graph.exec) (void)hipGraphExecDestroy(n->graph.exec);
  n->graph.exec = nullptr;
}

// The mode of a call, resolved once from the object's three settings and handed to its Run: the family the forward GEMMs run on
// (exact fp32, the f16x3 split, or one f16 MFMA per product, and with that one activations are f16 in memory), and whether the f16
// scale 2^-e is read from the device table the weight rebuild writes (training) or passed by value.  Training's own storage setting
// takes effect while the sampling side is plain fp32; under anything else a training call is refused (refuse_training).
enum { FORM_F32 = 0, FORM_H3 = 1, FORM_H1 = 2 };
struct Mode {
  int form = FORM_F32;
  bool table = false;
  bool h() const { return form == FORM_H1; }   // activations are f16
};
Mode mode_of(fdsr_nafnet n, bool training) {
  const bool plain = n->store == FDSR_NAF_STORE_F32 && n->prec == FDSR_PREC_F32;
  if (training) return n->train_store == FDSR_NAF_STORE_F16 && plain ? Mode{FORM_H1, true} : Mode{};
  return {n->store == FDSR_NAF_STORE_F16 ? FORM_H1 : n->prec == FDSR_PREC_F16X3 ? FORM_H3 : FORM_F32, false};
}
// some call reads the f16 forms of the weights (d_wq, d_hinv) and raises the range flag
bool f16_forms(fdsr_nafnet n) { return mode_of(n, false).form != FORM_F32 || mode_of(n, true).form != FORM_F32; }

int add_wt(fdsr_nafnet n, const std::string& key, std::vector<int64_t> shape) {
  WT w;
  w.key = key;
  w.shape = std::move(shape);
  n->wts.push_back(w);
  n->key2w[key] = (int)n->wts.size() - 1;
  return (int)n->wts.size() - 1;
}

int add_conv(fdsr_nafnet n, const std::string& name, int cin, int cout, int ks, int s, int p, bool bias, bool gate) {
  GemmL g;
  g.cin = cin; g.cout = cout; g.ks = ks; g.s = s; g.p = p; g.gate = gate;
  g.w = add_wt(n, name + ".weight", {cout, cin, ks, ks});
  if (bias) g.b = add_wt(n, name + ".bias", {cout});
  n->gemms.push_back(g);
  return (int)n->gemms.size() - 1;
}

// registration order of NAFBlock's state_dict: beta, gamma, mlp.1, conv1, conv2, conv3, sca.1, conv4, conv5, norm1.g, norm2.g
int add_block(fdsr_nafnet n, const std::string& name, int c) {
  BlockL b;
  b.name = name;
  b.c = c;
  b.beta = add_wt(n, name + ".beta", {1, c, 1, 1});
  b.gamma = add_wt(n, name + ".gamma", {1, c, 1, 1});
  b.mlpw = add_wt(n, name + ".mlp.1.weight", {4 * c, 2 * n->wd});
  b.mlpb = add_wt(n, name + ".mlp.1.bias", {4 * c});
  b.conv1 = add_conv(n, name + ".conv1", c, 2 * c, 1, 1, 0, true, false);
  b.dww = add_wt(n, name + ".conv2.weight", {2 * c, 1, 3, 3});
  b.dwb = add_wt(n, name + ".conv2.bias", {2 * c});
  b.conv3 = add_conv(n, name + ".conv3", c, c, 1, 1, 0, true, false);
  b.scaw = add_wt(n, name + ".sca.1.weight", {c, c, 1, 1});
  b.scab = add_wt(n, name + ".sca.1.bias", {c});
  b.conv4 = add_conv(n, name + ".conv4", c, 2 * c, 1, 1, 0, true, true);
  b.conv5 = add_conv(n, name + ".conv5", c, c, 1, 1, 0, true, false);
  b.g1 = add_wt(n, name + ".norm1.g", {1, c, 1, 1});
  b.g2 = add_wt(n, name + ".norm2.g", {1, c, 1, 1});
  b.row_off = n->R;
  n->R += 4 * c;
  n->blocks.push_back(b);
  return (int)n->blocks.size() - 1;
}

size_t take(size_t& off, size_t floats) {
  const size_t o = off;
  off += (floats + 63) / 64 * 64;   // 256-byte steps: every vector is float4-aligned
  return o;
}

void build_schema(fdsr_nafnet n) {
  const fdsr_nafnet_config& c = n->cfg;
  const int w = c.width;
  n->wd = w;
  n->L = c.n_levels;
  n->t1w = add_wt(n, "time_mlp.1.weight", {8 * w, w});
  n->t1b = add_wt(n, "time_mlp.1.bias", {8 * w});
  n->t2w = add_wt(n, "time_mlp.3.weight", {4 * w, 4 * w});
  n->t2b = add_wt(n, "time_mlp.3.bias", {4 * w});
  n->g_intro = add_conv(n, "intro", 2 * c.img_channel, w, 3, 1, 1, true, false);
  n->g_rcab0 = add_conv(n, "enhance.rcab.0", w, w, 3, 1, 1, true, false);
  n->g_rcab2 = add_conv(n, "enhance.rcab.2", w, w, 3, 1, 1, true, false);
  n->ca1w = add_wt(n, "enhance.rcab.3.attention.1.weight", {w / 16, w, 1, 1});
  n->ca1b = add_wt(n, "enhance.rcab.3.attention.1.bias", {w / 16});
  n->ca2w = add_wt(n, "enhance.rcab.3.attention.3.weight", {w, w / 16, 1, 1});
  n->ca2b = add_wt(n, "enhance.rcab.3.attention.3.bias", {w});
  n->g_ending = add_conv(n, "ending", w, c.img_channel, 3, 1, 1, true, false);
  n->enc.resize(n->L);
  n->dec.resize(n->L);
  int chan = w;
  for (int i = 0; i < n->L; ++i, chan *= 2)
    for (int j = 0; j < c.enc_blk_nums[i]; ++j) n->enc[i].push_back(add_block(n, "encoders." + std::to_string(i) + "." + std::to_string(j), chan));
  const int cmid = chan;
  for (int i = 0; i < n->L; ++i) {
    chan /= 2;
    for (int j = 0; j < c.dec_blk_nums[i]; ++j) n->dec[i].push_back(add_block(n, "decoders." + std::to_string(i) + "." + std::to_string(j), chan));
  }
  for (int j = 0; j < c.middle_blk_num; ++j) n->mid.push_back(add_block(n, "middle_blks." + std::to_string(j), cmid));
  chan = cmid;
  for (int i = 0; i < n->L; ++i, chan /= 2) n->ups.push_back(add_conv(n, "ups." + std::to_string(i) + ".0", chan, 2 * chan, 1, 1, 0, false, false));
  chan = w;
  for (int i = 0; i < n->L; ++i, chan *= 2) n->downs.push_back(add_conv(n, "downs." + std::to_string(i), chan, 2 * chan, 2, 2, 0, true, false));

  size_t off = 0;
  for (GemmL& g : n->gemms) {
    g.woff = take(off, (size_t)g.Kpad() * g.CoutPad());
    g.boff = take(off, g.CoutPad());
  }
  for (BlockL& b : n->blocks) {
    b.off_beta = take(off, b.c);
    b.off_gamma = take(off, b.c);
    b.off_dww = take(off, 18 * (size_t)b.c);
    b.off_dwb = take(off, 2 * b.c);
    b.off_scaw = take(off, (size_t)b.c * b.c);
    b.off_scab = take(off, b.c);
  }
  n->off_freq = take(off, w / 2);
  n->off_t1w = take(off, 8 * (size_t)w * w);
  n->off_t1b = take(off, 8 * w);
  n->off_t2w = take(off, 16 * (size_t)w * w);
  n->off_t2b = take(off, 4 * w);
  n->off_ca1w = take(off, (size_t)w * (w / 16));
  n->off_ca1b = take(off, w / 16);
  n->off_ca2w = take(off, (size_t)w * (w / 16));
  n->off_ca2b = take(off, w);
  n->off_rowsw = take(off, 2 * (size_t)w * n->R);
  n->off_rowsb = take(off, n->R);
  n->off_rowsadd = take(off, n->R);
  n->off_rowsmul = take(off, n->R);
  // training: the transposed convolutions (intro's, 64 -> 6, serves fdsr_nafnet_backward's d x / d cond only) and a zero bias for them
  int zmax = 64;
  for (const GemmL& g : n->gemms) {
    GemmL t;
    if (g.ks == 3) { t.cin = g.cout; t.cout = g.cin; t.ks = 3; t.s = 1; t.p = 1; }
    else if (g.ks == 2) { t.cin = g.cout; t.cout = 4 * g.cin; }
    else if (g.b < 0) { t.cin = g.cout / 4; t.cout = g.cin; t.ks = 2; t.s = 2; }
    else { t.cin = g.cout; t.cout = g.cin; }
    t.woff = take(off, (size_t)t.Kpad() * t.CoutPad());
    zmax = std::max(zmax, t.CoutPad());
    n->tgemms.push_back(t);
  }
  n->off_zero = take(off, zmax);
  for (GemmL& t : n->tgemms) t.boff = n->off_zero;
  n->arena_floats = off;
  for (GemmL& g : n->gemms) { g.hoff = n->hfrags; n->hfrags += g.hfrags(); g.hidx = (int)(&g - n->gemms.data()); }
  size_t po = 0;
  for (const WT& wt : n->wts) { n->poff.push_back(po); po += numel(wt.shape); }
  n->P = po;
}

// Every device form of the weights, written through a sink: FloatSink copies values from the host tensors (the upload), IndexSink
// records for every arena element the flat index of the master value it holds (-1: a constant), which is what the training
// step's device-side re-pack gathers through.
struct FloatSink {
  fdsr_nafnet n;
  std::vector<float>& a;
  void set(size_t ai, int wi, size_t ei) { a[ai] = n->wts[wi].host[ei]; }
  void cst(size_t ai, float v) { a[ai] = v; }
};
struct IndexSink {
  fdsr_nafnet n;
  std::vector<int>& a;
  void set(size_t ai, int wi, size_t ei) { a[ai] = (int)(n->poff[wi] + ei); }
  void cst(size_t, float) {}
};

template <class S>
void pack_forms(fdsr_nafnet n, S& s) {
  auto len = [&](int wi) { return numel(n->wts[wi].shape); };
  for (const GemmL& g : n->gemms) {
    const int Cp = g.CoutPad(), half = g.cout / 2;
    auto col = [&](int co) { return g.gate ? (co < half ? 64 * (co / 32) + co % 32 : 64 * ((co - half) / 32) + 32 + (co - half) % 32) : co; };
    for (int co = 0; co < g.cout; ++co) {
      const int pc = col(co);
      if (g.b >= 0) s.set(g.boff + pc, g.b, co);
      for (int ci = 0; ci < g.cin; ++ci)
        for (int ky = 0; ky < g.ks; ++ky)
          for (int kx = 0; kx < g.ks; ++kx)
            s.set(g.woff + ((size_t)(ky * g.ks + kx) * g.cin + ci) * Cp + pc, g.w, (((size_t)co * g.cin + ci) * g.ks + ky) * g.ks + kx);
    }
  }
  const int K2 = 2 * n->wd, R = n->R;
  for (const BlockL& b : n->blocks) {
    const int c = b.c;
    for (int i = 0; i < c; ++i) { s.set(b.off_beta + i, b.beta, i); s.set(b.off_gamma + i, b.gamma, i); s.set(b.off_scab + i, b.scab, i); }
    for (int ch = 0; ch < 2 * c; ++ch) {
      for (int k = 0; k < 9; ++k) s.set(b.off_dww + (size_t)k * 2 * c + ch, b.dww, (size_t)ch * 9 + k);
      s.set(b.off_dwb + ch, b.dwb, ch);
    }
    for (size_t i = 0; i < (size_t)c * c; ++i) s.set(b.off_scaw + i, b.scaw, i);
    // rows: [shift_att | scale_att | shift_ffn | scale_ffn], c each
    for (int r = 0; r < 4 * c; ++r) {
      const int gr = b.row_off + r, chunk = r / c, ch = r % c;
      for (int j = 0; j < K2; ++j) s.set(n->off_rowsw + (size_t)j * R + gr, b.mlpw, (size_t)r * K2 + j);
      s.set(n->off_rowsb + gr, b.mlpb, r);
      s.cst(n->off_rowsadd + gr, (chunk & 1) ? 1.f : 0.f);
      if (chunk == 1) s.set(n->off_rowsmul + gr, b.g1, ch);
      else if (chunk == 3) s.set(n->off_rowsmul + gr, b.g2, ch);
      else s.cst(n->off_rowsmul + gr, 1.f);
    }
  }
  // SinusoidalPosEmb: exp(arange(half) * -(log(10000) / (half - 1))) in fp32
  const int half = n->wd / 2;
  const float step = (float)(-(std::log(10000.0) / (half - 1)));
  for (int j = 0; j < half; ++j) s.cst(n->off_freq + j, expf((float)j * step));
  auto cp = [&](int wi, size_t off) { for (size_t i = 0; i < len(wi); ++i) s.set(off + i, wi, i); };
  cp(n->t1w, n->off_t1w); cp(n->t1b, n->off_t1b); cp(n->t2w, n->off_t2w); cp(n->t2b, n->off_t2b);
  cp(n->ca1w, n->off_ca1w); cp(n->ca1b, n->off_ca1b); cp(n->ca2w, n->off_ca2w); cp(n->ca2b, n->off_ca2b);
  // the input-gradient packs (training): the same GEMM kernel reads them as the weights of the transposed convolution
  for (size_t gi = 0; gi < n->gemms.size(); ++gi) {
    const GemmL& g = n->gemms[gi];
    const GemmL& t = n->tgemms[gi];
    const int Cp = t.CoutPad();
    for (int co = 0; co < g.cout; ++co)
      for (int ci = 0; ci < g.cin; ++ci)
        for (int ky = 0; ky < g.ks; ++ky)
          for (int kx = 0; kx < g.ks; ++kx) {
            const size_t src = (((size_t)co * g.cin + ci) * g.ks + ky) * g.ks + kx;
            size_t k, col;
            if (g.ks == 3) { k = (size_t)((2 - ky) * 3 + (2 - kx)) * g.cout + co; col = ci; }           // flipped taps
            else if (g.ks == 2) { k = co; col = (size_t)ci * 4 + ky * 2 + kx; }                         // downs: 1x1 + PixelShuffle scatter
            else if (g.b < 0) { k = (size_t)(co & 3) * (g.cout / 4) + (co >> 2); col = ci; }            // ups: 2x2 stride 2 over the shuffled gradient
            else { k = co; col = ci; }
            s.set(t.woff + k * Cp + col, g.w, src);
          }
  }
}

// FDSR_PREC_F16X3: the forward GEMMs' packed weights (arena `a`, as pack_forms wrote them) as hi = f16(w s), lo = f16(w s - hi) in
// the B-fragment order naf_gemm_h3_kernel loads.  s = 2^e <= 2^12 with max|w s| <= 2^15, the rule of the UNets' pack_weights_h: it
// keeps lo out of the f16 subnormal range for all but tiny weights, and the kernel multiplies the accumulator by 2^-e.
std::vector<uint16_t> split_weights(fdsr_nafnet n, const std::vector<float>& a) {
  std::vector<uint16_t> q(n->hfrags * 8, 0);
  auto bits = [](_Float16 v) { uint16_t b; memcpy(&b, &v, 2); return b; };
  for (GemmL& g : n->gemms) {
    const int Cp = g.CoutPad(), Kp = g.Kpad(), nk = g.K32() / HK;
    const float* w = a.data() + g.woff;
    float amax = 0.f;
    for (size_t i = 0; i < (size_t)Kp * Cp; ++i) amax = std::max(amax, std::min(std::fabs(w[i]), F16_MAX));
    int e = 12;
    if (amax > 0.f) e = std::min(12, (int)std::floor(std::log2(32768.0 / (double)amax)));
    const float scale = std::ldexp(1.0f, e);
    g.hinv = std::ldexp(1.0f, -e);
    for (int cot = 0; cot < Cp / BN; ++cot)
      for (int kc = 0; kc < nk; ++kc)
        for (int nb = 0; nb < 2; ++nb)
          for (int s = 0; s < 2; ++s)
            for (int l = 0; l < 64; ++l) {
              const size_t f = g.hoff + ((((size_t)cot * nk + kc) * 2 + nb) * 2 + s) * 2 * 64 + l;
              const int col = cot * BN + nb * 32 + (l & 31);
              for (int j = 0; j < 8; ++j) {
                const int k = kc * HK + 16 * s + 8 * (l >> 5) + j;
                const float v = k < Kp ? std::min(std::max(w[(size_t)k * Cp + col], -F16_MAX), F16_MAX) * scale : 0.f;
                const _Float16 hi = (_Float16)v;
                q[f * 8 + j] = bits(hi);
                q[(f + 64) * 8 + j] = bits((_Float16)(v - (float)hi));
              }
            }
  }
  return q;
}

// every device form from the host copies, one upload
int finalize(fdsr_nafnet n) {
  if (!n->dirty) return FDSR_OK;
  for (const WT& w : n->wts)
    if (!w.loaded) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet: tensor '%s' is missing", w.key.c_str());
  std::vector<float> a(n->arena_floats, 0.f);
  FloatSink sink{n, a};
  pack_forms(n, sink);
  if (!n->d_arena) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_arena), a.size() * sizeof(float)));
  HIPCHK(nullptr, hipDeviceSynchronize());   // nothing in flight reads the old forms
  HIPCHK(nullptr, hipMemcpy(n->d_arena, a.data(), a.size() * sizeof(float), hipMemcpyHostToDevice));
  if (f16_forms(n)) {
    const std::vector<uint16_t> q = split_weights(n, a);
    if (!n->d_wq) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_wq), q.size() * sizeof(uint16_t)));
    HIPCHK(nullptr, hipMemcpy(n->d_wq, q.data(), q.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    std::vector<float> hinv;
    for (const GemmL& g : n->gemms) hinv.push_back(g.hinv);
    if (!n->d_hinv) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_hinv), hinv.size() * sizeof(float)));
    HIPCHK(nullptr, hipMemcpy(n->d_hinv, hinv.data(), hinv.size() * sizeof(float), hipMemcpyHostToDevice));
    if (!n->d_sat) {
      HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_sat), 256));
      HIPCHK(nullptr, hipMemset(n->d_sat, 0, 256));
    }
  }
  n->dirty = false;
  n->table_valid = false;
  n->master_valid = false;
  return FDSR_OK;
}

// the host copies follow the device master again (a weight is about to be loaded over trained ones)
int host_from_master(fdsr_nafnet n) {
  if (!n->host_stale) return FDSR_OK;
  HIPCHK(nullptr, hipDeviceSynchronize());
  for (size_t i = 0; i < n->wts.size(); ++i)
    HIPCHK(nullptr, hipMemcpy(n->wts[i].host.data(), n->d_master + n->poff[i], n->wts[i].host.size() * sizeof(float), hipMemcpyDeviceToHost));
  n->host_stale = false;
  return FDSR_OK;
}

int nstrips_of(int HW) { return (HW + STRIP - 1) / STRIP; }

Plan make_plan(fdsr_nafnet n, int N, int H, int W) {
  Plan p{};
  const int pad = 1 << n->L, w = n->wd;
  p.N = N; p.H = H; p.W = W;
  p.Hp = round_up(H, pad);
  p.Wp = round_up(W, pad);
  const size_t M0 = (size_t)N * p.Hp * p.Wp;
  size_t off = 0;
  auto buf = [&](size_t floats) { const size_t o = off; off = align_up(off + floats * sizeof(float), 256); return o; };
  p.xin = buf(M0 * 6);
  p.A = buf(M0 * w);
  p.B = buf(M0 * w);
  p.T1 = buf(M0 * 2 * w);
  p.T2 = buf(M0 * w);
  p.stats = buf(M0 * 2);
  size_t part = 0;
  int cmax = w;
  for (int l = 0; l <= n->L; ++l) {
    part = std::max(part, (size_t)nstrips_of((p.Hp >> l) * (p.Wp >> l)) * ((size_t)w << l));
    cmax = w << l;
  }
  p.part = buf((size_t)N * part);
  p.sca = buf((size_t)N * cmax);
  p.ca = buf((size_t)N * w);
  p.tg = buf((size_t)N * 2 * w);
  p.trow = buf((size_t)N * n->R);
  p.eps = buf(M0 * 3);
  for (int l = 0; l < n->L; ++l) p.skip.push_back(buf((M0 * w) >> l));
  p.bytes = off;
  return p;
}

// A buffer of the walk and the type stored in it: fp32, or f16 elements in the first half of the slot.  sample_dst / train_dst say
// which where they hand the slots out, and every launch helper picks its kernel instance from its operands' h.  A plain float* --
// xin, eps, statistics, vectors, every gradient -- converts to an fp32 Act.  The activation slots of one NetDst are f16 exactly when
// its Run's mode is FORM_H1: sample_run and train_run, the only makers of a Run that walks, hand both the same Mode::h().
struct Act {
  float* p;
  bool h;
  Act(float* ptr = nullptr, bool f16 = false) : p(ptr), h(f16) {}
  operator float*() const { return p; }
  _Float16* f16() const { return reinterpret_cast<_Float16*>(p); }
};

// Where the forward walk (Run::net / Run::block) puts every tensor.  Sampling fills the table with aliases of four shared buffers
// (sample_dst), training with a slot per tensor its backward reads (train_dst in fdsr_nafnet_train.h).
template <class T> struct Slots { T out, st1, t1, t2, sca, y, st2, p4, g4; };   // a block's; st1 / st2: LayerNorm statistics, p4: conv4's pair before the gate
typedef Slots<Act> BlockDst;                                 // p4 null: not kept

struct NetDst {
  int N, H, W, Hp, Wp;
  Act xin, intro, r1, r, enh, eps;   // r1, r: the RCAB's two convolutions
  float *ca, *part, *tg, *trow;
  // per level i: downs[i]'s and ups[i]'s outputs; where encoder level i's skip and decoder step i's result are wanted -- a chain of
  // blocks that ends elsewhere (an empty list) is copied there; mid: the same for the middle blocks
  Act down[FDSR_NAFNET_MAX_LEVELS], up[FDSR_NAFNET_MAX_LEVELS], skip[FDSR_NAFNET_MAX_LEVELS], dec[FDSR_NAFNET_MAX_LEVELS], mid;
  std::vector<BlockDst> blk;
};

// A block may write over its input (out == input); its input and out may be none of y, t1, t2 -- except that the input may be y.
// downs[i] reads skip[i] and writes down[i]: the two are different buffers.  h: the activations are f16.
NetDst sample_dst(fdsr_nafnet n, bool h, int N, int H, int W, void* workspace) {
  const Plan pl = make_plan(n, N, H, W);
  auto F = [&](size_t off) { return reinterpret_cast<float*>(static_cast<char*>(workspace) + off); };
  const Act A{F(pl.A), h}, B{F(pl.B), h}, T1{F(pl.T1), h}, T2{F(pl.T2), h}, st{F(pl.stats)};
  NetDst d{};
  d.N = pl.N; d.H = pl.H; d.W = pl.W; d.Hp = pl.Hp; d.Wp = pl.Wp;
  d.xin = F(pl.xin); d.intro = B; d.r1 = T2; d.r = T1; d.ca = F(pl.ca); d.enh = A; d.eps = F(pl.eps); d.part = F(pl.part);
  d.tg = F(pl.tg); d.trow = F(pl.trow);
  d.blk.assign(n->blocks.size(), BlockDst{A, st, T1, T2, F(pl.sca), B, st, Act{}, T2});
  d.mid = A;
  for (int i = 0; i < n->L; ++i) {
    d.down[i] = d.dec[i] = A; d.up[i] = B; d.skip[i] = Act{F(pl.skip[i]), h};
    if (!n->enc[i].empty()) d.blk[n->enc[i].back()].out = d.skip[i];
  }
  return d;
}

typedef void (*GemmFn)(GemmArgs);
template <int PRO, bool VEC> GemmFn gemm_fn(int form) {
  return form == FORM_H1 ? naf_gemm_h1_kernel<PRO, VEC> : form == FORM_H3 ? naf_gemm_h3_kernel<PRO, VEC> : naf_gemm_kernel<PRO, VEC>;
}

// A GEMM's prologue (1x1 convolutions only: k is the input channel) and epilogue, as GemmArgs names their operands
struct Pro { int kind = PRO_NONE; const float *pmul = nullptr, *padd = nullptr; int pstride = 0; const float* stats = nullptr; };
struct Epi { int kind = EPI_BIAS; const float *res = nullptr, *evec = nullptr; float* out2 = nullptr; };
inline Pro ln(const float* stats, const float* mul, const float* add, int stride) { return {PRO_LN, mul, add, stride, stats}; }
inline Pro scaled(const float* vec, int stride) { return {PRO_MUL, vec, nullptr, stride}; }
inline Epi residual(const float* res, const float* evec) { return {EPI_RES, res, evec}; }   // out = res + v evec[co]
inline Epi gated(float* pair) { return {EPI_GATE, nullptr, nullptr, pair}; }                // pair: kept before the gate (training), or null
inline Epi shuffled(const float* skip) { return {EPI_PSHUF, skip}; }                        // out = PixelShuffle(v) + skip

struct Run {
  fdsr_nafnet n;
  Mode m;     // mode_of(n, is this a training call); d's slots were handed out for it
  NetDst d;
  hipStream_t st;
  const float* rows;   // the blocks' time rows, image b at rows + b * rstride
  int rstride;
  const char* stop = nullptr;   // debug tap: stop after this tensor
  bool hit = false;
  Act tap_at;
  int tap_h = 0, tap_w = 0, tap_c = 0;
  int err = FDSR_OK;

  const float* P(size_t off) const { return n->d_arena + off; }
  static unsigned nb(size_t total) { return (unsigned)((total + 255) / 256); }
  void check() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess && err == FDSR_OK) err = fail(nullptr, FDSR_E_HIP, "fdsr_nafnet: kernel launch failed: %s", hipGetErrorString(e));
  }
  template <class K, class... A> void launch(K kernel, dim3 grid, dim3 block, size_t lds, A... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    check();
  }
  // operands whose stored types do not fit the kernel a helper would pick: a mistake in this file, never a caller's -- made loud
  bool misfit(bool bad) {
    if (bad && err == FDSR_OK) err = fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet: internal error: an operand's stored type does not fit its kernel");
    return bad;
  }
  void copy(Act dst, Act src, size_t elems) {   // between slots of one stored type
    if (misfit(dst.h != src.h)) return;
    (void)hipMemcpyAsync(dst, src, elems * (src.h ? sizeof(_Float16) : sizeof(float)), hipMemcpyDeviceToDevice, st);
    check();
  }
  bool tap(const std::string& name, Act at, int h, int w, int c) {
    if (err != FDSR_OK) return true;
    if (stop && name == stop) { hit = true; tap_at = at; tap_h = h; tap_w = w; tap_c = c; return true; }
    return false;
  }

  // A forward GEMM runs on the mode's family.
  void gemm(int gi, Act x, Act out, int Hin, int Win, Pro pro = {}, Epi epi = {}) { gemm_l(n->gemms[gi], m.form, x, out, Hin, Win, pro, epi); }

  // The family fixes how the kernel reads: naf_gemm_h1_kernel takes x (but for intro's fp32 xin, the one input with cin % 8), res and
  // out2 as f16, the other two take them as fp32; only out's type is an argument (o32, which H1 alone reads).  x is checked against
  // that; res and out2 are slots of the same NetDst as x and out (see Act) and travel as plain pointers.
  void gemm_l(const GemmL& g, int form, Act x, Act out, int Hin, int Win, Pro pro, Epi epi) {
    if (misfit(g.cin % 8 == 0 && x.h != (form == FORM_H1))) return;
    GemmArgs a{};
    a.x = x; a.w = P(g.woff); a.bias = P(g.boff); a.out = out; a.out2 = epi.out2;
    a.stats = pro.stats; a.pmul = pro.pmul; a.padd = pro.padd; a.res = epi.res; a.evec = epi.evec;
    a.N = d.N; a.Hin = Hin; a.Win = Win; a.Cin = g.cin;
    a.Hout = (Hin + 2 * g.p - g.ks) / g.s + 1;
    a.Wout = (Win + 2 * g.p - g.ks) / g.s + 1;
    a.Cout = g.cout; a.KW = g.ks; a.S = g.s; a.P = g.p; a.K = g.K(); a.Kpad = g.Kpad(); a.CoutPad = g.CoutPad();
    a.ostride = epi.kind == EPI_GATE ? g.cout / 2 : epi.kind == EPI_PSHUF ? g.cout / 4 : g.cout;
    a.pstride = pro.pstride; a.epi = epi.kind;
    const int M = d.N * a.Hout * a.Wout;
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(a.CoutPad / BN));
    if (form != FORM_F32) {
      a.wq = n->d_wq + g.hoff; a.winv = g.hinv; a.sat = n->d_sat;
      a.o32 = form == FORM_H1 && !out.h;
      if (m.table) a.winvp = n->d_hinv + g.hidx;
    }
    const GemmFn k = g.cin % 8 ? gemm_fn<PRO_NONE, false>(form) : pro.kind == PRO_LN ? gemm_fn<PRO_LN, true>(form)
                     : pro.kind == PRO_MUL ? gemm_fn<PRO_MUL, true>(form) : gemm_fn<PRO_NONE, true>(form);
    launch(k, grid, dim3(NT), 0, a);
  }

  void ln_stats(Act x, float* stats, int M, int C) {
    if (x.h) launch(naf_ln_stats_h_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, x.f16(), stats, M, C);
    else launch(naf_ln_stats_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, x, stats, M, C);
  }
  void dw_gate(const BlockL& b, Act x, Act y, int h, int w, int ns) {
    const int c = b.c;
    if (x.h) {
      int lp_shift = 3;   // 2^lp_shift lanes, two channels each, cover a pixel: 8 (c = 16) .. 64
      while (lp_shift < 6 && (2 << lp_shift) < c) ++lp_shift;
      launch(naf_dw_gate_h_kernel, dim3((unsigned)ns, (unsigned)((c + (2 << lp_shift) - 1) / (2 << lp_shift)), (unsigned)d.N), dim3(256), 0, x.f16(),
             P(b.off_dww), P(b.off_dwb), y.f16(), d.part, h, w, c, ns, lp_shift, n->d_sat);
    } else launch(naf_dw_gate_kernel, dim3((unsigned)ns, (unsigned)((c + 63) / 64), (unsigned)d.N), dim3(256), 0, x, P(b.off_dww), P(b.off_dwb), y,
                d.part, h, w, c, ns);
  }
  void chansum(Act r, int HW, int ns) {   // the RCAB's pool: per-strip sums of r [N][HW][wd] into d.part
    const int wd = n->wd;
    if (r.h) launch(naf_chansum_h_kernel, dim3((unsigned)ns, (unsigned)((wd + 127) / 128), (unsigned)d.N), dim3(256), 0, r.f16(), d.part, HW, wd, ns);
    else launch(naf_chansum_kernel, dim3((unsigned)ns, (unsigned)((wd + 63) / 64), (unsigned)d.N), dim3(256), 0, r, d.part, HW, wd, ns);
  }

  void block(int bi, Act cur, int h, int w) {
    const BlockL& b = n->blocks[bi];
    const BlockDst& s = d.blk[bi];
    const int c = b.c, HW = h * w, M = d.N * HW, ns = nstrips_of(HW);
    const float* rw = rows + b.row_off;
    ln_stats(cur, s.st1, M, c);
    gemm(b.conv1, cur, s.t1, h, w, ln(s.st1, rw + c, rw, rstride));
    dw_gate(b, s.t1, s.t2, h, w, ns);
    launch(naf_sca_kernel, dim3((unsigned)((c + 15) / 16), (unsigned)d.N), dim3(256), (c + 256) * sizeof(float), d.part, ns, HW, P(b.off_scaw),
           P(b.off_scab), s.sca, c);
    gemm(b.conv3, s.t2, s.y, h, w, scaled(s.sca, c), residual(cur, P(b.off_beta)));
    ln_stats(s.y, s.st2, M, c);
    gemm(b.conv4, s.y, s.g4, h, w, ln(s.st2, rw + 3 * c, rw + 2 * c, rstride), gated(s.p4));
    gemm(b.conv5, s.g4, s.out, h, w, {}, residual(s.y, P(b.off_gamma)));
  }

  // the blocks of `list` from cur on; the result is wanted at `want` and copied there if the chain ended elsewhere.  False: stop (a tap, an error)
  bool chain(const std::vector<int>& list, Act cur, Act want, int h, int w, int c) {
    for (int bi : list) {
      block(bi, cur, h, w);
      cur = d.blk[bi].out;
      if (tap(n->blocks[bi].name, cur, h, w, c)) return false;
    }
    if (cur.p != want.p) copy(want, cur, (size_t)d.N * h * w * c);
    return true;
  }

  // the network up to `ending` (padded NHWC [N][Hp][Wp][3] in d.eps); xin is staged already
  void net() {
    const int wd = n->wd, L = n->L;
    int h = d.Hp, w = d.Wp, c = wd;
    gemm(n->g_intro, d.xin, d.intro, h, w);
    if (tap("intro", d.intro, h, w, wd)) return;
    gemm(n->g_rcab0, d.intro, d.r1, h, w, {}, {EPI_RELU});
    gemm(n->g_rcab2, d.r1, d.r, h, w);
    const int HW = h * w, ns = nstrips_of(HW);
    chansum(d.r, HW, ns);
    launch(naf_ca_kernel, dim3((unsigned)d.N), dim3(256), (wd + 256 + wd / 16) * sizeof(float), d.part, ns, HW, P(n->off_ca1w), P(n->off_ca1b),
           P(n->off_ca2w), P(n->off_ca2b), d.ca, wd, wd / 16);
    const size_t total = (size_t)d.N * HW * wd;
    if (d.intro.h) launch(naf_enhance_h_kernel, dim3(nb(total / 8)), dim3(256), 0, d.intro.f16(), d.r.f16(), d.ca, d.enh.f16(), HW, wd, total / 8, n->d_sat);
    else launch(naf_enhance_kernel, dim3(nb(total)), dim3(256), 0, d.intro, d.r, d.ca, d.enh, HW, wd, total);
    if (tap("enhance", d.enh, h, w, wd)) return;
    for (int i = 0; i < L; ++i) {
      if (!chain(n->enc[i], i ? d.down[i - 1] : d.enh, d.skip[i], h, w, c)) return;
      gemm(n->downs[i], d.skip[i], d.down[i], h, w);
      h /= 2; w /= 2; c *= 2;
      if (tap("downs." + std::to_string(i), d.down[i], h, w, c)) return;
    }
    if (!chain(n->mid, d.down[L - 1], d.mid, h, w, c)) return;
    for (int i = 0; i < L; ++i) {
      gemm(n->ups[i], i ? d.dec[i - 1] : d.mid, d.up[i], h, w, {}, shuffled(d.skip[L - 1 - i]));
      h *= 2; w *= 2; c /= 2;
      if (tap("ups." + std::to_string(i), d.up[i], h, w, c)) return;
      if (!chain(n->dec[i], d.up[i], d.dec[i], h, w, c)) return;
    }
    gemm(n->g_ending, d.dec[L - 1], d.eps, h, w);
    tap("ending", d.eps, h, w, n->cfg.img_channel);
  }

  void prep(const float* x, const float* cond) {
    const size_t total = (size_t)d.N * d.Hp * d.Wp;
    launch(naf_prep_kernel, dim3(nb(total)), dim3(256), 0, x, cond, d.xin, d.H, d.W, d.Hp, d.Wp, total);
  }

  // time rows of `count` time values (device) into dst [count][R]; tg: scratch [count][2 wd]
  void time_rows(const float* time_dev, int count, float* tg, float* dst) {
    const int wd = n->wd;
    launch(naf_time_kernel, dim3((unsigned)count), dim3(256), 17 * wd * sizeof(float), time_dev, P(n->off_freq), P(n->off_t1w), P(n->off_t1b),
           P(n->off_t2w), P(n->off_t2b), tg, wd);
    launch(naf_rows_kernel, dim3((unsigned)((n->R + 255) / 256), (unsigned)count), dim3(256), 0, tg, P(n->off_rowsw), P(n->off_rowsb),
           P(n->off_rowsadd), P(n->off_rowsmul), dst, 2 * wd, n->R);
  }

  // one forward at per-image times (device): their rows, xin, the walk
  void forward(const float* x, const float* cond, const float* time_dev) {
    time_rows(time_dev, d.N, d.tg, d.trow);
    rows = d.trow;
    prep(x, cond);
    net();
  }

  void tail(int mode, float* x, const float* cond, const float* noise, float* traj, unsigned long long seed, long long first,
            const int32_t* tiles = nullptr, int scene_w = 0) {
    StepTables tb{};
    if (mode) {
      tb.theta = n->d_sde;
      tb.sigma = n->d_sde + (n->T + 1);
      tb.sbar = n->d_sde + 2 * (n->T + 1);
      tb.dt = n->dt;
      tb.sqrt_dt = (float)std::sqrt((double)n->dt);
      tb.T = n->T;
    }
    const size_t total = (size_t)d.N * d.H * d.W;
    launch(naf_tail_kernel, dim3(nb(total)), dim3(256), 0, d.eps, x, cond, noise, traj, n->d_ctl, tb, seed, first, tiles, scene_w, mode, d.H, d.W, d.Hp,
           d.Wp, total);
  }
};

size_t plan_bytes(fdsr_nafnet n, int N, int H, int W) { return make_plan(n, N, H, W).bytes; }

// What every call that runs the network checks first: the shape limits, the weights (finalize), the workspace against the bytes of
// the call's plan (plan_bytes, train_plan_bytes), asked for once the shape is known to be good.
int check_args(fdsr_nafnet n, const char* fn, int batch, int height, int width, void* ws, size_t ws_bytes,
               size_t (*need_bytes)(fdsr_nafnet, int, int, int)) {
  if (!n || batch < 1 || height < 1 || width < 1 || !ws) return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, batch, height, width);
  if ((size_t)batch * round_up(height, 1 << n->L) * round_up(width, 1 << n->L) * 2 * n->wd >= (1ull << 31) || batch > 65535)
    return fail(nullptr, FDSR_E_INVALID, "%s: B %d at %dx%d exceeds the 32-bit pixel indexing of the kernels", fn, batch, height, width);
  const int rc = finalize(n);
  if (rc) return rc;
  const size_t need = need_bytes(n, batch, height, width);
  if (ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 255))
    return fail(nullptr, FDSR_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes) or not 256-byte aligned", fn, ws_bytes, need);
  return FDSR_OK;
}

int ensure_table(fdsr_nafnet n, hipStream_t st) {
  if (n->table_valid) return FDSR_OK;
  const int cnt = n->T + 1;
  float *times = nullptr, *tg = nullptr;
  if (!n->d_rowtable) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_rowtable), (size_t)cnt * n->R * sizeof(float)));
  if (!n->d_cur_row) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_cur_row), (size_t)n->R * sizeof(float)));
  if (!n->d_ctl) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_ctl), 256));
  HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&times), cnt * sizeof(float)));
  HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&tg), (size_t)cnt * 2 * n->wd * sizeof(float)));
  Run r{n, Mode{}, NetDst{}, st, nullptr, 0};   // the time kernels only
  r.launch(naf_iota_kernel, dim3(Run::nb(cnt)), dim3(256), 0, times, cnt);
  r.time_rows(times, cnt, tg, n->d_rowtable);
  const hipError_t e = hipStreamSynchronize(st);   // once per (weights, schedule): the scratch is freed below
  (void)hipFree(times);
  (void)hipFree(tg);
  if (r.err) return r.err;
  HIPCHK(nullptr, e);
  n->table_valid = true;
  return FDSR_OK;
}

// the Run of a checked sampling-side call, over sampling's shared buffers
Run sample_run(fdsr_nafnet n, int batch, int height, int width, void* workspace, hipStream_t st, const float* rows, int rstride) {
  const Mode m = mode_of(n, false);
  return Run{n, m, sample_dst(n, m.h(), batch, height, width, workspace), st, rows, rstride};
}

// What the three mode setters do once the argument is good.  The device forms are rebuilt from the fp32 master through pack_forms by
// the next call that runs (finalize: the split planes, the table of scales); after optimizer steps the master is on the device.
int switch_mode(fdsr_nafnet n, int* setting, int mode, const char* killer) {
  if (mode == *setting) return FDSR_OK;
  const int rc = host_from_master(n);
  if (rc) return rc;
  *setting = mode; n->dirty = true;
  kill_ticket(n, killer);
  drop_graph(n);
  return FDSR_OK;
}

// Training calls run while the sampling side is plain fp32 (the device-side re-pack writes the fp32 forms and, under f16 training
// storage, the planes of that mode only).  hint: name the setter that leads back, as the calls that run the network do.
int refuse_training(fdsr_nafnet n, const char* fn, bool hint) {
  const int form = mode_of(n, false).form;
  if (form == FORM_H1)
    return fail(nullptr, FDSR_E_INVALID, "%s: training runs on fp32 activations only, the object is in FDSR_NAF_STORE_F16, f16 storage%s", fn,
                hint ? " (fdsr_nafnet_set_storage)" : "");
  if (form == FORM_H3)
    return fail(nullptr, FDSR_E_INVALID, "%s: training runs in FDSR_PREC_F32 only, the object is in f16x3%s", fn, hint ? " (fdsr_nafnet_set_precision)" : "");
  return FDSR_OK;
}

}  // namespace

#include "fdsr_nafnet_train.h"

extern "C" {

int fdsr_nafnet_create(const fdsr_nafnet_config* cfg, fdsr_nafnet* out) {
  if (!cfg || !out) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_create: null argument");
  if (cfg->img_channel != 3 || cfg->width < 16 || cfg->width % 16 || cfg->n_levels < 1 || cfg->n_levels > FDSR_NAFNET_MAX_LEVELS ||
      cfg->middle_blk_num < 0 || ((long long)cfg->width << cfg->n_levels) > 8192)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_create: unsupported configuration (img_channel %d, width %d, %d levels)", cfg->img_channel,
                cfg->width, cfg->n_levels);
  for (int i = 0; i < cfg->n_levels; ++i)
    if (cfg->enc_blk_nums[i] < 0 || cfg->dec_blk_nums[i] < 0 || cfg->enc_blk_nums[i] > 64 || cfg->dec_blk_nums[i] > 64)
      return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_create: bad block count at level %d", i);
  fdsr_nafnet n = new (std::nothrow) fdsr_nafnet_obj();
  if (!n) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_create: out of host memory");
  n->cfg = *cfg;
  build_schema(n);
  *out = n;
  return FDSR_OK;
}

void fdsr_nafnet_destroy(fdsr_nafnet n) {
  if (!n) return;
  drop_graph(n);
  for (void* p : {(void*)n->d_arena, (void*)n->d_sde, (void*)n->d_rowtable, (void*)n->d_cur_row, (void*)n->d_ctl, (void*)n->d_master,
                  (void*)n->d_grad, (void*)n->d_m, (void*)n->d_v, (void*)n->d_cum, (void*)n->d_map, (void*)n->d_rowmap, (void*)n->d_wq,
                  (void*)n->d_sat, (void*)n->d_hinv, n->d_hdesc})
    if (p) (void)hipFree(p);
  if (n->h_sat) (void)hipHostFree(n->h_sat);
  delete n;
}

int fdsr_nafnet_num_weights(fdsr_nafnet n) { return n ? (int)n->wts.size() : fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_num_weights: null object"); }

int fdsr_nafnet_weight_info(fdsr_nafnet n, int index, char* key, int key_capacity, int64_t* shape4, int* ndim) {
  if (!n || index < 0 || index >= (int)n->wts.size() || !key || key_capacity < 1 || !shape4 || !ndim)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_weight_info: bad arguments");
  const WT& w = n->wts[index];
  if ((int)w.key.size() + 1 > key_capacity) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_weight_info: key buffer too small");
  memcpy(key, w.key.c_str(), w.key.size() + 1);
  *ndim = (int)w.shape.size();
  for (size_t i = 0; i < w.shape.size(); ++i) shape4[i] = w.shape[i];
  return FDSR_OK;
}

int fdsr_nafnet_load_weight(fdsr_nafnet n, const char* key, const float* host_f32, const int64_t* shape, int ndim) {
  if (!n || !key || !host_f32 || (ndim > 0 && !shape) || ndim < 0) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_load_weight: bad arguments");
  const auto it = n->key2w.find(key);
  if (it == n->key2w.end()) return fail(nullptr, FDSR_E_KEY, "fdsr_nafnet_load_weight: unknown tensor '%s'", key);
  const int rc = host_from_master(n);   // after an optimizer step the other tensors' host copies are refreshed first
  if (rc) return rc;
  WT& w = n->wts[it->second];
  if (ndim != (int)w.shape.size() || !std::equal(w.shape.begin(), w.shape.end(), shape))
    return fail(nullptr, FDSR_E_KEY, "fdsr_nafnet_load_weight: '%s' has the wrong shape", key);
  w.host.assign(host_f32, host_f32 + numel(w.shape));
  w.loaded = true;
  n->dirty = true;
  n->table_valid = false;
  kill_ticket(n, "fdsr_nafnet_load_weight (a weight load)");
  drop_graph(n);
  return FDSR_OK;
}

int fdsr_nafnet_weights_complete(fdsr_nafnet n) {
  if (!n) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_weights_complete: null object");
  for (const WT& w : n->wts)
    if (!w.loaded) return 0;
  return 1;
}

int fdsr_nafnet_set_precision(fdsr_nafnet n, int mode) {
  if (!n || (mode != FDSR_PREC_F32 && mode != FDSR_PREC_F16X3))
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_set_precision: mode must be FDSR_PREC_F32 (0) or FDSR_PREC_F16X3 (1), not %d", mode);
  if (mode == FDSR_PREC_F16X3 && n->store == FDSR_NAF_STORE_F16)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_set_precision: FDSR_PREC_F16X3 while the storage is FDSR_NAF_STORE_F16: set the storage back "
                                         "first (fdsr_nafnet_set_storage)");
  return switch_mode(n, &n->prec, mode, "fdsr_nafnet_set_precision (a precision switch)");
}

int fdsr_nafnet_set_storage(fdsr_nafnet n, int mode) {
  if (!n || (mode != FDSR_NAF_STORE_F32 && mode != FDSR_NAF_STORE_F16))
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_set_storage: mode must be FDSR_NAF_STORE_F32 (0) or FDSR_NAF_STORE_F16 (1), not %d", mode);
  if (mode == FDSR_NAF_STORE_F16 && n->prec == FDSR_PREC_F16X3)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_set_storage: FDSR_NAF_STORE_F16 while the precision is FDSR_PREC_F16X3: set the precision "
                                         "back first (fdsr_nafnet_set_precision)");
  return switch_mode(n, &n->store, mode, "fdsr_nafnet_set_storage (a storage switch)");
}

int fdsr_nafnet_set_train_storage(fdsr_nafnet n, int mode) {
  if (!n || (mode != FDSR_NAF_STORE_F32 && mode != FDSR_NAF_STORE_F16))
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_set_train_storage: mode must be FDSR_NAF_STORE_F32 (0) or FDSR_NAF_STORE_F16 (1), not %d", mode);
  return switch_mode(n, &n->train_store, mode, "fdsr_nafnet_set_train_storage (a storage switch)");
}

int fdsr_nafnet_check_saturation(fdsr_nafnet n, void* hip_stream) {
  if (!n) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_check_saturation: null object");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(nullptr, hipStreamSynchronize(st));
  if (!f16_forms(n) || !n->d_sat) return FDSR_OK;
  if (!n->h_sat) HIPCHK(nullptr, hipHostMalloc(reinterpret_cast<void**>(&n->h_sat), 64, hipHostMallocDefault));
  *n->h_sat = 0;
  HIPCHK(nullptr, hipMemcpyAsync(n->h_sat, n->d_sat, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(nullptr, hipStreamSynchronize(st));
  if (!*n->h_sat) return FDSR_OK;
  HIPCHK(nullptr, hipMemsetAsync(n->d_sat, 0, sizeof(int), st));
  if (mode_of(n, false).h())
    return fail(nullptr, FDSR_E_SATURATED, "f16 storage: an activation of the NAFNet exceeded the f16 range (+-65504) and was clamped; "
                                           "re-run this call after fdsr_nafnet_set_storage(FDSR_NAF_STORE_F32)");
  if (mode_of(n, true).h())
    return fail(nullptr, FDSR_E_SATURATED, "f16 training storage: an activation of the NAFNet exceeded the f16 range (+-65504) and was clamped; "
                                           "the gradients of this call are not to be used: skip the step, or train after "
                                           "fdsr_nafnet_set_train_storage(FDSR_NAF_STORE_F32)");
  return fail(nullptr, FDSR_E_SATURATED, "f16x3: a GEMM input of the NAFNet exceeded the f16 range (+-65504) and was clamped; "
                                         "re-run this call after fdsr_nafnet_set_precision(FDSR_PREC_F32)");
}

int fdsr_nafnet_set_sde(fdsr_nafnet n, int T, const float* thetas, const float* sigmas, const float* sigma_bars, float dt) {
  if (!n || T < 1 || T > (1 << 20) || !thetas || !sigmas || !sigma_bars || !(dt > 0.f))
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_set_sde: bad arguments (T %d)", T);
  drop_graph(n);
  HIPCHK(nullptr, hipDeviceSynchronize());
  for (float** p : {&n->d_sde, &n->d_rowtable})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  n->T = T;
  n->dt = dt;
  n->thetas.assign(thetas, thetas + T + 1);
  n->sigmas.assign(sigmas, sigmas + T + 1);
  n->sbars.assign(sigma_bars, sigma_bars + T + 1);
  n->cum_T = 0;   // thetas_cumsum belongs to the schedule it was given with
  std::vector<float> all(n->thetas);
  all.insert(all.end(), n->sigmas.begin(), n->sigmas.end());
  all.insert(all.end(), n->sbars.begin(), n->sbars.end());
  HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_sde), all.size() * sizeof(float)));
  HIPCHK(nullptr, hipMemcpy(n->d_sde, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
  n->table_valid = false;
  return FDSR_OK;
}

int fdsr_nafnet_workspace_bytes(fdsr_nafnet n, int batch, int height, int width, size_t* bytes) {
  if (!n || !bytes || batch < 1 || height < 1 || width < 1)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_workspace_bytes: bad arguments (B %d, %dx%d)", batch, height, width);
  *bytes = plan_bytes(n, batch, height, width);
  return FDSR_OK;
}

int fdsr_nafnet_forward(fdsr_nafnet n, const float* x_nchw, const float* cond_nchw, const float* time_dev, float* out_nchw, int batch,
                        int height, int width, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!x_nchw || !cond_nchw || !time_dev || !out_nchw) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_forward: null tensor");
  const int rc = check_args(n, "fdsr_nafnet_forward", batch, height, width, workspace, workspace_bytes, plan_bytes);
  if (rc) return rc;
  Run r = sample_run(n, batch, height, width, workspace, reinterpret_cast<hipStream_t>(hip_stream), nullptr, n->R);
  r.forward(x_nchw, cond_nchw, time_dev);
  r.tail(0, out_nchw, nullptr, nullptr, nullptr, 0, 0);
  return r.err;
}

int fdsr_nafnet_debug_tensor(fdsr_nafnet n, const char* name, const float* x_nchw, const float* cond_nchw, const float* time_dev,
                             int batch, int height, int width, float* out_nhwc, size_t capacity_floats, int* dims3, void* workspace,
                             size_t workspace_bytes, void* hip_stream) {
  if (!name || !x_nchw || !cond_nchw || !time_dev || !out_nhwc || !dims3) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_debug_tensor: null argument");
  const int rc = check_args(n, "fdsr_nafnet_debug_tensor", batch, height, width, workspace, workspace_bytes, plan_bytes);
  if (rc) return rc;
  Run r = sample_run(n, batch, height, width, workspace, reinterpret_cast<hipStream_t>(hip_stream), nullptr, n->R);
  r.stop = name;
  r.forward(x_nchw, cond_nchw, time_dev);
  if (r.err) return r.err;
  if (!r.hit) return fail(nullptr, FDSR_E_KEY, "fdsr_nafnet_debug_tensor: unknown tap '%s'", name);
  const size_t count = (size_t)batch * r.tap_h * r.tap_w * r.tap_c;
  if (count > capacity_floats) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_debug_tensor: '%s' needs %zu floats", name, count);
  dims3[0] = r.tap_h; dims3[1] = r.tap_w; dims3[2] = r.tap_c;
  if (r.tap_at.h) {   // the stored f16 values, widened
    r.launch(naf_widen_h_kernel, dim3(Run::nb(count)), dim3(256), 0, r.tap_at.f16(), out_nhwc, count);
    return r.err;
  }
  HIPCHK(nullptr, hipMemcpyAsync(out_nhwc, r.tap_at, count * sizeof(float), hipMemcpyDeviceToDevice, r.st));
  return FDSR_OK;
}

int fdsr_nafnet_sample(fdsr_nafnet n, const float* state_nchw, const float* cond_nchw, const float* noise, uint64_t seed,
                       int64_t first_image, int flags, float* out_nchw, float* traj, int batch, int height, int width,
                       void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!state_nchw || !cond_nchw || !out_nchw || first_image < 0 || (flags & ~(FDSR_SAMPLE_GRAPH | FDSR_NAFNET_ODE)))
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_sample: bad arguments");
  if (n && n->T < 1) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_sample: no schedule (fdsr_nafnet_set_sde)");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const bool use_graph = flags & FDSR_SAMPLE_GRAPH;
  if (use_graph && !st) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_sample: FDSR_SAMPLE_GRAPH needs a created stream");
  int rc = check_args(n, "fdsr_nafnet_sample", batch, height, width, workspace, workspace_bytes, plan_bytes);
  if (rc) return rc;
  if ((rc = ensure_table(n, st))) return rc;
  const int mode = (flags & FDSR_NAFNET_ODE) ? 2 : 1;
  // the table counts where the call draws its own noise: explicit noise and the ODE draw nothing
  NoiseTiles call_tiles;
  if (n->noise_tiles.origins && first_image != 0)   // two ways to place an image in a larger whole: one at a time
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_sample: first_image must be 0 under a noise-tile table (got %lld)", (long long)first_image);
  if (!noise && mode == 1 && !n->noise_tiles.for_call(batch, width, &call_tiles))
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_sample: %d images under a noise-tile table of %d", batch, n->noise_tiles.n);
  const int32_t* tiles = call_tiles.origins;
  const int scene_w = call_tiles.scene_w;
  HIPCHK(nullptr, hipMemcpyAsync(out_nchw, state_nchw, (size_t)batch * 3 * height * width * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIPCHK(nullptr, hipMemsetAsync(n->d_ctl, 0, sizeof(int), st));
  Run r = sample_run(n, batch, height, width, workspace, st, n->d_cur_row, 0);
  auto step = [&]() -> int {
    r.launch(naf_row_copy_kernel, dim3(Run::nb(n->R)), dim3(256), 0, n->d_rowtable, n->d_cur_row, n->d_ctl, n->T, n->R);
    r.prep(out_nchw, cond_nchw);
    r.net();
    r.tail(mode, out_nchw, cond_nchw, noise, traj, seed, first_image, tiles, scene_w);
    r.launch(naf_advance_kernel, dim3(1), dim3(64), 0, n->d_ctl);
    return r.err;
  };
  if (!use_graph) {
    for (int k = 0; k < n->T; ++k)
      if ((rc = step())) return rc;
    return FDSR_OK;
  }
  auto& g = n->graph;
  if (!(g.exec && g.cond == cond_nchw && g.noise == noise && g.out == out_nchw && g.traj == traj && g.ws == workspace && g.N == batch &&
        g.H == height && g.W == width && g.flags == flags && g.seed == seed && g.first == first_image && g.tiles == tiles && g.scene_w == scene_w)) {
    drop_graph(n);
    hipGraphExec_t exec = nullptr;
    if ((rc = capture_exec(nullptr, st, step, &exec))) return rc;
    g.cond = cond_nchw; g.noise = noise; g.out = out_nchw; g.traj = traj; g.ws = workspace;
    g.N = batch; g.H = height; g.W = width; g.flags = flags; g.seed = seed; g.first = first_image; g.tiles = tiles; g.scene_w = scene_w; g.exec = exec;
  }
  for (int k = 0; k < n->T; ++k) HIPCHK(nullptr, hipGraphLaunch(g.exec, st));
  return FDSR_OK;
}

int fdsr_nafnet_randn(float* dst_nchw, int batch, int height, int width, int plane, uint64_t seed, int64_t first_image, void* hip_stream) {
  if (!dst_nchw || batch < 1 || height < 1 || width < 1 || plane < 0 || first_image < 0)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_randn: bad arguments");
  const size_t HW = (size_t)height * width, total = (size_t)batch * HW;
  hipLaunchKernelGGL(naf_randn_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), dst_nchw,
                     (int)HW, plane, (unsigned long long)seed, (size_t)first_image * HW, total, (const int*)nullptr, 0, width);
  HIPCHK(nullptr, hipGetLastError());
  return FDSR_OK;
}

int fdsr_nafnet_set_noise_tiles(fdsr_nafnet n, const int32_t* origins_dev, int n_tiles, int scene_w) {
  if (!n || !n->noise_tiles.set(origins_dev, n_tiles, scene_w))
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_set_noise_tiles: a table needs n_tiles >= 1 and scene_w >= 1 (got %d, %d)", n_tiles, scene_w);
  return FDSR_OK;
}

int fdsr_nafnet_randn_tiles(float* dst_nchw, int batch, int height, int width, int plane, uint64_t seed, const int32_t* origins_dev,
                            int scene_w, void* hip_stream) {
  if (!dst_nchw || !origins_dev || batch < 1 || height < 1 || width < 1 || plane < 0 || scene_w < 1)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_randn_tiles: bad arguments");
  const size_t HW = (size_t)height * width, total = (size_t)batch * HW;
  hipLaunchKernelGGL(naf_randn_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), dst_nchw,
                     (int)HW, plane, (unsigned long long)seed, (size_t)0, total, origins_dev, scene_w, width);
  HIPCHK(nullptr, hipGetLastError());
  return FDSR_OK;
}

int fdsr_upscale_bicubic_f32(const float* src_nchw, float* dst_nchw, int batch, int channels, int height, int width, int scale,
                             void* hip_stream) {
  if (!src_nchw || !dst_nchw || batch < 1 || channels < 1 || height < 1 || width < 1 || scale < 1 || scale > 64)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_upscale_bicubic_f32: bad arguments");
  const size_t total = (size_t)batch * channels * height * width * scale * scale;
  hipLaunchKernelGGL(naf_upscale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), src_nchw,
                     dst_nchw, height, width, scale, total);
  HIPCHK(nullptr, hipGetLastError());
  return FDSR_OK;
}

}  // extern "C"
