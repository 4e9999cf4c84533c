// SwinIR (MSI_SR_model/model/swinir.py: GeneratorResNet, upsampler='pixelshuffle', resi_connection='1conv', patch_size 1, ape=False)
// inference in exact fp32 on gfx950.
//
//   x    = (reflect_pad(img, to a multiple of the window) - mean) * img_range              NCHW -> NHWC       swin_input_kernel
//   f    = conv_first(x);  t = patch_embed.norm(f)
//   per RSTB: depth Swin blocks  { t += proj(window_attention(qkv(norm1(t))));  t += fc2(gelu(fc1(norm2(t)))) },  t = conv(t) + t_in
//   y    = conv_after_body(norm(t)) + f;  y = leaky_relu(conv_before_upsample(y), 0.01)
//   y    = pixel_shuffle(conv(y)) per factor of two (one conv + PixelShuffle(3) at scale 3);  out = conv_last(y) / img_range + mean,
//          cropped to (H * scale, W * scale), stored NCHW
//
// Activations are fp32 NHWC throughout: a [B][H][W][C] feature map is the [B][H W][C] token matrix, so PatchEmbed / PatchUnEmbed,
// the roll and the window partition never move data (the attention kernel folds the last two into its addresses).
//
// Three kernel families:
//   swin_gemm_kernel   out[M][N] = gather(A)[M][K] . W[K][N] + bias on v_mfma_f32_32x32x2_f32; the gather (token rows / 3x3
//                      implicit GEMM with a zero halo) and the epilogue (none / erf-GELU / LeakyReLU / + residual / pixel-shuffle
//                      store / + mean, crop, NCHW) are template parameters.  Weights are packed [Kpad][Npad] on the host.
//   swin_ln_kernel     LayerNorm over C (biased variance, eps 1e-5), one wave per token.
//   swin_attn_kernel   one workgroup per (image, window), a loop over the heads: S = (q scale) k^T + bias + mask in LDS, row
//                      softmax, O = P V; head_dim padded to 32 for the MFMAs.
// Every output element has one fixed summation order (no atomics, no split-K): reruns are bitwise equal and an image's result
// depends neither on B nor on its place in the batch.
//
// The network is written once, as a walk (Walker below): the same code lists the checkpoint tensors in load order, sizes the
// workspace and launches the kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fdsr_engine_int.h"

using namespace fdsr_int;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 64, BK = 16, NT = 256;
constexpr int AP = BM + 32;   // LDS row pitches: the two k rows an MFMA operand read touches sit 32 banks apart
constexpr int BP = BN + 32;
constexpr int WS = 8, WT = WS * WS;   // the window and its tokens
constexpr int HD = 32;                // head_dim padded to the MFMA tile
constexpr int TP = WT + 32;           // pitch of the [k][token] operand arrays of the attention kernel
constexpr int NBUF = 6;
constexpr int NUM_FEAT = 64;          // channels of the reconstruction tail
constexpr int LN_MAX_C = 512;         // swin_ln_kernel keeps a row in 8 registers per lane

enum Gather { ROWS = 0, CONV3 = 1 };
enum Epi { EPI_NONE = 0, EPI_GELU = 1, EPI_LRELU = 2, EPI_RES = 3, EPI_SHUFFLE = 4, EPI_NCHW = 5 };

struct GemmArgs {
  const float* x;      // ROWS: [M][K];  CONV3: NHWC [B][H][W][Cin]
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

// One workgroup: BM rows x BN columns; 4 waves in a 2 x 2 grid, each 64 rows x 32 columns (two 32x32 accumulators).  Thread t
// stages row t % BM and k-octet t / BM of every BK chunk (registers prefetch the next chunk while the MFMAs run on this one).
// Rows >= M, out-of-image taps and k >= K read as zero.  VEC: Cin % 4 == 0 (ROWS: K % 4 == 0), so a quad of k is 4 consecutive
// floats of one row / tap, 16-byte aligned.
template <int GATHER, int EPI, bool VEC>
__global__ void __launch_bounds__(NT) swin_gemm_kernel(GemmArgs p) {
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
  const int bk = t >> 4, bn = (t & 15) * 4;

  // the address of element k of this thread's row, or null where it reads as zero
  auto src = [&](int k) -> const float* {
    if (!mval || k >= p.K) return nullptr;
    if (GATHER == ROWS) return p.x + (size_t)gm * p.K + k;
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

  // epilogue: C/D map col = lane & 31 (column), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
  const int co = n0 + wn * 32 + r31;
  if (co >= p.N) return;
  const float bias = p.bias[co];
  const int HW = p.H * p.W;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int om = m0 + wm * 64 + mb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
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

// (Shifted-)window attention of one (image, window): a loop over the heads.  Token (ty, tx) of window (wy, wx) is the pixel
// ((wy 8 + ty + shift) mod H, (wx 8 + tx + shift) mod W) -- torch.roll by -shift, then window_partition -- and the output goes
// back to the same pixel (window_reverse, the roll by +shift).  qkv: [B][H W][3 C], a token's row is q | k | v, each head-major.
// biasT: [heads][j][i] = relative_position_bias_table[index(i, j)][head].  shift > 0: tokens of different regions of the rolled
// image (three slices per axis: [0, H - 8), [H - 8, H - shift), [H - shift, H)) get -100 added, as calculate_mask does.
__global__ void __launch_bounds__(256) swin_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ biasT, float* __restrict__ out,
                                                        int H, int W, int C, int heads, int hd, int shift, float scale) {
  __shared__ float sQt[HD * TP];   // [d][token], q * scale
  __shared__ float sKt[HD * TP];   // [d][token]
  __shared__ float sV[WT * HD];    // [token][d]
  __shared__ float sSt[WT * TP];   // [j][i]: the scores of query i against key j, then the probabilities
  __shared__ float sRed[4 * WT];
  __shared__ int sPix[WT], sRid[WT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nwx = W / WS, nwy = H / WS;
  const int win = blockIdx.x % (nwx * nwy), b = blockIdx.x / (nwx * nwy);
  const int wy = win / nwx, wx = win - wy * nwx;
  if (t < WT) {
    const int ys = wy * WS + (t >> 3), xs = wx * WS + (t & 7);
    sPix[t] = ((ys + shift) % H) * W + (xs + shift) % W;
    const int rh = ys < H - WS ? 0 : ys < H - shift ? 1 : 2, rw = xs < W - WS ? 0 : xs < W - shift ? 1 : 2;
    sRid[t] = shift > 0 ? rh * 3 + rw : 0;
  }
  __syncthreads();
  const size_t img = (size_t)b * H * W;
  const int r31 = lane & 31, h = lane >> 5;

  for (int head = 0; head < heads; ++head) {
    // stage: q, k by token (lane = token: conflict-free transposed stores), v by channel (lane = d: coalesced reads)
    {
      const float* row = qkv + (img + sPix[lane]) * 3 * C + head * hd;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int d = wave * 8 + e;
        sQt[d * TP + lane] = d < hd ? row[d] * scale : 0.f;
        sKt[d * TP + lane] = d < hd ? row[C + d] : 0.f;
      }
      const int d = t & 31;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int tok = (t >> 5) + 8 * e;
        sV[tok * HD + d] = d < hd ? qkv[(img + sPix[tok]) * 3 * C + 2 * C + head * hd + d] : 0.f;
      }
    }
    __syncthreads();
    // St[j][i] = sum_d k[j][d] q[i][d]: wave (wj, wi) owns one 32 x 32 tile; rows are keys so that the stores run along i
    {
      const int wj = wave >> 1, wi = wave & 1;
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int s = 0; s < HD / 2; ++s) {
        const int kr = 2 * s + h;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sKt[kr * TP + wj * 32 + r31], sQt[kr * TP + wi * 32 + r31], acc, 0, 0, 0);
      }
      const int i = wi * 32 + r31;
      const int ri = sRid[i];
      const float* bh = biasT + (size_t)head * WT * WT;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = wj * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float v = acc[r] + bh[j * WT + i];
        if (sRid[j] != ri) v += -100.f;
        sSt[j * TP + i] = v;
      }
    }
    __syncthreads();
    // row softmax: thread (quarter, i) covers keys [16 quarter, 16 quarter + 16); the four partial results combine in order
    {
      const int i = lane, j0 = wave * 16;
      float m = sSt[j0 * TP + i];
#pragma unroll
      for (int j = 1; j < 16; ++j) m = fmaxf(m, sSt[(j0 + j) * TP + i]);
      sRed[wave * WT + i] = m;
      __syncthreads();
      m = fmaxf(fmaxf(sRed[i], sRed[WT + i]), fmaxf(sRed[2 * WT + i], sRed[3 * WT + i]));
      __syncthreads();
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float e = expf(sSt[(j0 + j) * TP + i] - m);
        sSt[(j0 + j) * TP + i] = e;
        s += e;
      }
      sRed[wave * WT + i] = s;
      __syncthreads();
      s = ((sRed[i] + sRed[WT + i]) + sRed[2 * WT + i]) + sRed[3 * WT + i];
#pragma unroll
      for (int j = 0; j < 16; ++j) sSt[(j0 + j) * TP + i] = sSt[(j0 + j) * TP + i] / s;
    }
    __syncthreads();
    // O[i][d] = sum_j P[i][j] v[j][d]: waves 0 and 1 own 32 queries each
    if (wave < 2) {
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int s = 0; s < WT / 2; ++s) {
        const int kr = 2 * s + h;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sSt[kr * TP + wave * 32 + r31], sV[kr * HD + r31], acc, 0, 0, 0);
      }
      if (r31 < hd) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          out[(img + sPix[i]) * C + head * hd + r31] = acc[r];
        }
      }
    }
    __syncthreads();   // the next head overwrites the operands
  }
}

// save_img1: (x * 255).clamp(0, 255) truncated to uint8; NCHW -> NHWC
__global__ void __launch_bounds__(256) swin_to_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ y, int HW, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % 3);
  const size_t pix = i / 3, b = pix / HW, q = pix - b * HW;
  const float v = fminf(fmaxf(__fmul_rn(x[(b * 3 + c) * HW + q], 255.f), 0.f), 255.f);
  y[i] = (unsigned char)(int)v;
}

enum Kind { LINEAR, CONV, LNORM, RPB };

// One named module of the checkpoint: LINEAR / CONV / LNORM own name.weight and name.bias, RPB owns the tensor `name` itself
struct LayerDesc {
  std::string name;
  Kind kind;
  int cin, cout;   // LNORM: cout = C;  RPB: cout = heads
  int K() const { return kind == CONV ? 9 * cin : cin; }
  int Kpad() const { return round_up(K(), BK); }
  int Npad() const { return round_up(cout, BN); }
  int tensors() const { return kind == RPB ? 1 : 2; }
  std::string tensor_name(int j) const { return kind == RPB ? name : name + (j == 0 ? ".weight" : ".bias"); }
  std::vector<int64_t> shape(int j) const {
    if (kind == RPB) return {(2 * WS - 1) * (2 * WS - 1), cout};
    if (j == 1 || kind == LNORM) return {cout};
    if (kind == CONV) return {cout, cin, 3, 3};
    return {cout, cin};
  }
};

// A tensor in a workspace buffer: [N][H][W][C]
struct T { int buf, H, W, C; };

enum Mode { TABLE, SIZE, RUN };

struct Walker {
  Mode mode;
  fdsr_swinir_config cfg{};
  std::vector<LayerDesc>* table = nullptr;      // TABLE: appended to
  std::vector<std::string>* taps = nullptr;     // TABLE: the tap names, appended to
  size_t need[NBUF] = {};                       // SIZE: floats per image of each buffer
  int N = 0, Hin = 0, Win = 0;
  const float* img = nullptr;                   // RUN: the input, NCHW
  float* dst = nullptr;                         // RUN: the output, NCHW (null: a debug walk, which ends at `stop`)
  float* buf[NBUF] = {};
  float* const* w = nullptr;
  float* const* b = nullptr;
  hipStream_t st = nullptr;
  int li = 0;                                   // the next layer's index (load order)
  const char* stop = nullptr;                   // RUN: the tap to end at
  bool done = false;
  T tapped{};
  int err = FDSR_OK;

  bool live() const { return mode == RUN && err == FDSR_OK && !done; }
  void touch(const T& t) { need[t.buf] = std::max(need[t.buf], (size_t)t.H * t.W * t.C); }
  void check(hipError_t e) {
    if (e != hipSuccess && err == FDSR_OK) err = fail(nullptr, FDSR_E_HIP, "fdsr_swinir: kernel launch failed: %s", hipGetErrorString(e));
  }
  void tap(const std::string& name, const T& t) {
    if (mode == TABLE) taps->push_back(name);
    if (live() && stop && name == stop) { done = true; tapped = t; }
  }
  int layer(const std::string& name, Kind kind, int cin, int cout) {
    if (mode == TABLE) table->push_back(LayerDesc{name, kind, cin, cout});
    return li++;
  }

  template <int GATHER, int EPI>
  void launch_gemm(const GemmArgs& a, bool vec) {
    const dim3 grid((unsigned)((a.M + BM - 1) / BM), (unsigned)(a.Npad / BN));
    if (vec) hipLaunchKernelGGL((swin_gemm_kernel<GATHER, EPI, true>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((swin_gemm_kernel<GATHER, EPI, false>), grid, dim3(NT), 0, st, a);
    check(hipGetLastError());
  }

  // out = epilogue(gather(in) . W + bias).  res: the EPI_RES addend.  r: the EPI_SHUFFLE factor.
  T gemm(const std::string& name, Kind kind, int epi, const T& in, int cout, int ob, const T* res = nullptr, int r = 1) {
    const int idx = layer(name, kind, in.C, cout);
    T out{ob, in.H * r, in.W * r, cout / (r * r)};
    if (mode == SIZE && epi != EPI_NCHW) touch(out);
    if (!live()) return out;
    const LayerDesc L{name, kind, in.C, cout};
    GemmArgs a{};
    a.x = buf[in.buf];
    a.w = w[idx];
    a.bias = b[idx];
    a.res = res ? buf[res->buf] : nullptr;
    a.out = epi == EPI_NCHW ? dst : buf[ob];
    a.M = N * in.H * in.W;
    a.N = cout;
    a.K = L.K();
    a.Kpad = L.Kpad();
    a.Npad = L.Npad();
    a.H = in.H;
    a.W = in.W;
    a.Cin = in.C;
    a.r = r;
    a.Hc = Hin * cfg.upscale;
    a.Wc = Win * cfg.upscale;
    a.slope = 0.01f;   // nn.LeakyReLU()'s default
    a.range = cfg.img_range;
    for (int c = 0; c < 3; ++c) a.mean[c] = cfg.mean[c];
    const bool vec = in.C % 4 == 0;
    if (kind == LINEAR) {
      if (epi == EPI_NONE) launch_gemm<ROWS, EPI_NONE>(a, vec);
      else if (epi == EPI_GELU) launch_gemm<ROWS, EPI_GELU>(a, vec);
      else launch_gemm<ROWS, EPI_RES>(a, vec);
    } else {
      if (epi == EPI_NONE) launch_gemm<CONV3, EPI_NONE>(a, vec);
      else if (epi == EPI_LRELU) launch_gemm<CONV3, EPI_LRELU>(a, vec);
      else if (epi == EPI_RES) launch_gemm<CONV3, EPI_RES>(a, vec);
      else if (epi == EPI_SHUFFLE) launch_gemm<CONV3, EPI_SHUFFLE>(a, vec);
      else launch_gemm<CONV3, EPI_NCHW>(a, vec);
    }
    return out;
  }

  T norm(const std::string& name, const T& in, int ob) {
    const int idx = layer(name, LNORM, in.C, in.C);
    T out{ob, in.H, in.W, in.C};
    if (mode == SIZE) touch(out);
    if (!live()) return out;
    const int M = N * in.H * in.W;
    hipLaunchKernelGGL(swin_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, buf[in.buf], w[idx], b[idx], buf[ob], M, in.C);
    check(hipGetLastError());
    return out;
  }

  // attention over the q | k | v rows of `qkv`, into `ob`
  T attention(const std::string& name, const T& qkv, int heads, int shift, int ob) {
    const int idx = layer(name, RPB, 0, heads);
    const int C = qkv.C / 3;
    T out{ob, qkv.H, qkv.W, C};
    if (mode == SIZE) touch(out);
    if (!live()) return out;
    const int hd = C / heads;
    const unsigned blocks = (unsigned)(N * (qkv.H / WS) * (qkv.W / WS));
    hipLaunchKernelGGL(swin_attn_kernel, dim3(blocks), dim3(256), 0, st, buf[qkv.buf], w[idx], buf[ob], qkv.H, qkv.W, C, heads, hd, shift,
                       1.f / sqrtf((float)hd));
    check(hipGetLastError());
    return out;
  }

  // The whole network.  Buffers: 0 the packed input, 1 conv_first's output (kept for conv_after_body), 2 / 3 the tokens (an
  // RSTB's input stays in 2 while its blocks work in 3), 4 a LayerNorm's or the attention's output, 5 qkv / the MLP's hidden
  // rows; the reconstruction tail alternates between 4 and 5.
  void walk() {
    const int C = cfg.embed_dim;
    const int Hp = round_up(std::max(Hin, 1), WS), Wp = round_up(std::max(Win, 1), WS);
    T x{0, Hp, Wp, 3};
    if (mode == SIZE) touch(x);
    if (live()) {
      const size_t total = (size_t)N * Hp * Wp * 3;
      hipLaunchKernelGGL(swin_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, img, buf[0], Hin, Win, Hp, Wp, cfg.mean[0],
                         cfg.mean[1], cfg.mean[2], cfg.img_range, total);
      check(hipGetLastError());
    }
    const T f = gemm("conv_first", CONV, EPI_NONE, x, C, 1);
    tap("conv_first", f);
    T a{2, Hp, Wp, C};
    if (cfg.patch_norm) {
      a = norm("patch_embed.norm", f, 2);
    } else {
      if (mode == SIZE) touch(a);
      if (live()) check(hipMemcpyAsync(buf[2], buf[1], (size_t)N * Hp * Wp * C * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    tap("patch_embed.norm", a);
    for (int i = 0; i < cfg.n_layers; ++i) {
      const std::string lp = "layers." + std::to_string(i);
      T cur = a;
      for (int j = 0; j < cfg.depths[i]; ++j) {
        const std::string bp = lp + ".residual_group.blocks." + std::to_string(j), tp = lp + ".blocks." + std::to_string(j);
        T n1 = norm(bp + ".norm1", cur, 4);
        T qkv = gemm(bp + ".attn.qkv", LINEAR, EPI_NONE, n1, 3 * C, 5);
        T o = attention(bp + ".attn.relative_position_bias_table", qkv, cfg.num_heads[i], j % 2 ? WS / 2 : 0, 4);
        T y = gemm(bp + ".attn.proj", LINEAR, EPI_RES, o, C, 3, &cur);
        tap(tp + ".attn", y);
        T n2 = norm(bp + ".norm2", y, 4);
        T hid = gemm(bp + ".mlp.fc1", LINEAR, EPI_GELU, n2, cfg.mlp_hidden, 5);
        cur = gemm(bp + ".mlp.fc2", LINEAR, EPI_RES, hid, C, 3, &y);
        tap(tp + ".mlp", cur);
      }
      a = gemm(lp + ".conv", CONV, EPI_RES, cur, C, 2, &a);
      tap(lp, a);
    }
    T n = norm("norm", a, 4);
    T y = gemm("conv_after_body", CONV, EPI_RES, n, C, 3, &f);
    tap("conv_after_body", y);
    y = gemm("conv_before_upsample.0", CONV, EPI_LRELU, y, NUM_FEAT, 4);
    int ob = 5;
    if (cfg.upscale == 3) {
      y = gemm("upsample.0", CONV, EPI_SHUFFLE, y, 9 * NUM_FEAT, ob, nullptr, 3);
      tap("upsample.0", y);
    } else {
      for (int k = 0; (1 << k) < cfg.upscale; ++k, ob = 9 - ob) {
        y = gemm("upsample." + std::to_string(2 * k), CONV, EPI_SHUFFLE, y, 4 * NUM_FEAT, ob, nullptr, 2);
        tap("upsample." + std::to_string(k), y);
      }
    }
    gemm("conv_last", CONV, EPI_NCHW, y, 3, 0);
  }
};

struct Plan { size_t off[NBUF]; size_t bytes; };

struct Graph { int B, H, W; const void *x, *out, *ws; hipGraphExec_t exec; };

}  // namespace

struct fdsr_swinir_obj {
  fdsr_swinir_config cfg{};
  std::vector<LayerDesc> table;
  std::vector<std::string> taps;
  std::vector<unsigned char> have;   // [layer * 2 + j]
  std::vector<float*> w, b;          // device: LINEAR / CONV packed [Kpad][Npad] + bias [Npad]; LNORM gamma + beta; RPB biasT [heads][64][64]
  std::vector<Graph> graphs;
};

namespace {

Walker walker(fdsr_swinir s, Mode mode, int B, int H, int W) {
  Walker wk{mode};
  wk.cfg = s->cfg;
  wk.N = B;
  wk.Hin = H;
  wk.Win = W;
  return wk;
}

Plan make_plan(fdsr_swinir s, int B, int H, int W) {
  Walker wk = walker(s, SIZE, B, H, W);
  wk.walk();
  Plan pl{};
  size_t off = 0;
  for (int i = 0; i < NBUF; ++i) {
    pl.off[i] = off;
    off = align_up(off + (size_t)B * wk.need[i] * sizeof(float), 256);
  }
  pl.bytes = off;
  return pl;
}

void drop_graphs(fdsr_swinir s) {
  for (Graph& g : s->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  s->graphs.clear();
}

// F.pad's rule for 'reflect': the padding must be smaller than the side it mirrors
int check_shape(const char* fn, int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, B, H, W);
  const int ph = round_up(H, WS) - H, pw = round_up(W, WS) - W;
  if (ph >= H || pw >= W)
    return fail(nullptr, FDSR_E_INVALID, "%s: a %dx%d image cannot be reflect-padded by (%d, %d) to a multiple of the window", fn, H, W, ph, pw);
  return FDSR_OK;
}

// everything a forward or a debug walk checks, then the walker ready to run
int prepare(fdsr_swinir s, const char* fn, const float* x, int B, int H, int W, void* ws, size_t ws_bytes, void* stream, Walker* out) {
  if (!s || !x || !ws) return fail(nullptr, FDSR_E_INVALID, "%s: null argument", fn);
  int rc = check_shape(fn, B, H, W);
  if (rc) return rc;
  for (size_t L = 0; L < s->table.size(); ++L)
    for (int j = 0; j < s->table[L].tensors(); ++j)
      if (!s->have[L * 2 + j]) return fail(nullptr, FDSR_E_STATE, "%s: tensor '%s' is missing", fn, s->table[L].tensor_name(j).c_str());
  const Plan pl = make_plan(s, B, H, W);
  if (ws_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(ws) & 255))
    return fail(nullptr, FDSR_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes) or not 256-byte aligned", fn, ws_bytes, pl.bytes);
  Walker wk = walker(s, RUN, B, H, W);
  wk.img = x;
  for (int i = 0; i < NBUF; ++i) wk.buf[i] = reinterpret_cast<float*>(static_cast<char*>(ws) + pl.off[i]);
  wk.w = s->w.data();
  wk.b = s->b.data();
  wk.st = reinterpret_cast<hipStream_t>(stream);
  *out = wk;
  return FDSR_OK;
}

}  // namespace

extern "C" {

int fdsr_swinir_create(const fdsr_swinir_config* cfg, fdsr_swinir* out) {
  if (!cfg || !out) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: null argument");
  const fdsr_swinir_config& c = *cfg;
  if (c.window_size != WS) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: window_size %d is not supported (8 only)", c.window_size);
  if (c.n_layers < 1 || c.n_layers > FDSR_SWINIR_MAX_LAYERS)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: %d layers (1..%d)", c.n_layers, FDSR_SWINIR_MAX_LAYERS);
  if (c.embed_dim < 1 || c.embed_dim > LN_MAX_C || c.mlp_hidden < 1)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: embed_dim %d (1..%d), mlp hidden width %d", c.embed_dim, LN_MAX_C, c.mlp_hidden);
  for (int i = 0; i < c.n_layers; ++i) {
    if (c.depths[i] < 1 || c.num_heads[i] < 1 || c.embed_dim % c.num_heads[i])
      return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: layer %d: depth %d, embed_dim %d over %d heads", i, c.depths[i], c.embed_dim,
                  c.num_heads[i]);
    if (c.embed_dim / c.num_heads[i] > HD)
      return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: layer %d: head_dim %d is not supported (at most %d)", i,
                  c.embed_dim / c.num_heads[i], HD);
  }
  if (c.upscale != 2 && c.upscale != 3 && c.upscale != 4 && c.upscale != 8)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: upscale %d is not supported (2, 3, 4, 8)", c.upscale);
  if (!(c.img_range > 0.f)) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: img_range must be positive");
  fdsr_swinir s = new (std::nothrow) fdsr_swinir_obj();
  if (!s) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: out of host memory");
  s->cfg = c;
  Walker wk = walker(s, TABLE, 1, WS, WS);
  wk.table = &s->table;
  wk.taps = &s->taps;
  wk.walk();
  s->have.assign(s->table.size() * 2, 0);
  s->w.assign(s->table.size(), nullptr);
  s->b.assign(s->table.size(), nullptr);
  *out = s;
  return FDSR_OK;
}

void fdsr_swinir_destroy(fdsr_swinir s) {
  if (!s) return;
  drop_graphs(s);
  for (float* p : s->w)
    if (p) (void)hipFree(p);
  for (float* p : s->b)
    if (p) (void)hipFree(p);
  delete s;
}

int fdsr_swinir_load(fdsr_swinir s, const char* name, const float* host_f32, const int64_t* shape, int ndim) {
  if (!s || !name || !host_f32 || (ndim > 0 && !shape) || ndim < 0) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_load: bad arguments");
  int layer = -1, j = -1;
  for (size_t L = 0; L < s->table.size() && layer < 0; ++L)
    for (int q = 0; q < s->table[L].tensors(); ++q)
      if (s->table[L].tensor_name(q) == name) { layer = (int)L; j = q; break; }
  if (layer < 0) return fail(nullptr, FDSR_E_KEY, "fdsr_swinir_load: unknown tensor '%s'", name);
  const LayerDesc& L = s->table[layer];
  const std::vector<int64_t> want = L.shape(j);
  if (ndim != (int)want.size() || !std::equal(want.begin(), want.end(), shape))
    return fail(nullptr, FDSR_E_KEY, "fdsr_swinir_load: '%s' has the wrong shape", name);
  std::vector<float> packed;
  if (L.kind == RPB) {
    // biasT[head][j][i] = table[(yi - yj + 7) * 15 + (xi - xj + 7)][head]: the gather of relative_position_index, once
    packed.resize((size_t)L.cout * WT * WT);
    for (int hh = 0; hh < L.cout; ++hh)
      for (int kj = 0; kj < WT; ++kj)
        for (int qi = 0; qi < WT; ++qi) {
          const int idx = ((qi >> 3) - (kj >> 3) + WS - 1) * (2 * WS - 1) + ((qi & 7) - (kj & 7) + WS - 1);
          packed[((size_t)hh * WT + kj) * WT + qi] = host_f32[(size_t)idx * L.cout + hh];
        }
  } else if (L.kind == LNORM) {
    packed.assign(host_f32, host_f32 + L.cout);
  } else if (j == 1) {
    packed.assign((size_t)L.Npad(), 0.f);
    std::copy(host_f32, host_f32 + L.cout, packed.begin());
  } else {
    // [Kpad][Npad]; rows K..Kpad-1 and columns cout..Npad-1 stay zero
    const int Np = L.Npad();
    packed.assign((size_t)L.Kpad() * Np, 0.f);
    if (L.kind == LINEAR) {
      for (int co = 0; co < L.cout; ++co)
        for (int ci = 0; ci < L.cin; ++ci) packed[(size_t)ci * Np + co] = host_f32[(size_t)co * L.cin + ci];
    } else {
      for (int co = 0; co < L.cout; ++co)
        for (int ci = 0; ci < L.cin; ++ci)
          for (int tp = 0; tp < 9; ++tp) packed[((size_t)tp * L.cin + ci) * Np + co] = host_f32[((size_t)co * L.cin + ci) * 9 + tp];
    }
  }
  float*& dst = j == 0 ? s->w[layer] : s->b[layer];
  // a running forward may still read the old values: loading is host-synchronous, as in the sibling families
  HIPCHK(nullptr, hipDeviceSynchronize());
  drop_graphs(s);
  if (!dst) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&dst), packed.size() * sizeof(float)));
  HIPCHK(nullptr, hipMemcpy(dst, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
  s->have[(size_t)layer * 2 + j] = 1;
  return FDSR_OK;
}

int fdsr_swinir_workspace_bytes(fdsr_swinir s, int batch, int height, int width, size_t* bytes) {
  if (!s || !bytes) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_workspace_bytes: null argument");
  const int rc = check_shape("fdsr_swinir_workspace_bytes", batch, height, width);
  if (rc) return rc;
  *bytes = make_plan(s, batch, height, width).bytes;
  return FDSR_OK;
}

int fdsr_swinir_forward(fdsr_swinir s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace,
                        size_t workspace_bytes, void* hip_stream, int flags) {
  if (!out_nchw || (flags & ~FDSR_SWINIR_GRAPH)) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_forward: bad arguments");
  if ((flags & FDSR_SWINIR_GRAPH) && !hip_stream)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_forward: FDSR_SWINIR_GRAPH needs a created stream");
  Walker wk{RUN};
  int rc = prepare(s, "fdsr_swinir_forward", x_nchw, batch, height, width, workspace, workspace_bytes, hip_stream, &wk);
  if (rc) return rc;
  wk.dst = out_nchw;
  if (!(flags & FDSR_SWINIR_GRAPH)) {
    wk.walk();
    return wk.err;
  }
  // one graph per (B, H, W); other pointers under the same shape capture anew
  Graph* g = nullptr;
  for (Graph& q : s->graphs)
    if (q.B == batch && q.H == height && q.W == width) g = &q;
  if (g && !(g->x == x_nchw && g->out == out_nchw && g->ws == workspace)) {
    (void)hipGraphExecDestroy(g->exec);
    s->graphs.erase(s->graphs.begin() + (g - s->graphs.data()));
    g = nullptr;
  }
  if (!g) {
    hipGraphExec_t exec = nullptr;
    if ((rc = capture_exec(nullptr, wk.st, [&]() -> int { wk.walk(); return wk.err; }, &exec))) return rc;
    s->graphs.push_back(Graph{batch, height, width, x_nchw, out_nchw, workspace, exec});
    g = &s->graphs.back();
  }
  HIPCHK(nullptr, hipGraphLaunch(g->exec, wk.st));
  return FDSR_OK;
}

int fdsr_swinir_debug_tensor(fdsr_swinir s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                             size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!name || !out_nhwc || !dims3) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_debug_tensor: null argument");
  Walker wk{RUN};
  const int rc = prepare(s, "fdsr_swinir_debug_tensor", x_nchw, batch, height, width, workspace, workspace_bytes, hip_stream, &wk);
  if (rc) return rc;
  // the name is checked before anything runs: a walk that meets no tap would end in conv_last's store
  const bool known = std::find(s->taps.begin(), s->taps.end(), std::string(name)) != s->taps.end();
  if (!known) return fail(nullptr, FDSR_E_KEY, "fdsr_swinir_debug_tensor: unknown tap '%s'", name);
  wk.stop = name;
  wk.walk();
  if (wk.err) return wk.err;
  if (!wk.done) return fail(nullptr, FDSR_E_KEY, "fdsr_swinir_debug_tensor: tap '%s' was not reached", name);
  const T& tp = wk.tapped;
  const size_t count = (size_t)batch * tp.H * tp.W * tp.C;
  if (count > capacity_floats) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_debug_tensor: '%s' needs %zu floats", name, count);
  dims3[0] = tp.H; dims3[1] = tp.W; dims3[2] = tp.C;
  HIPCHK(nullptr, hipMemcpyAsync(out_nhwc, wk.buf[tp.buf], count * sizeof(float), hipMemcpyDeviceToDevice, wk.st));
  return FDSR_OK;
}

int fdsr_swinir_to_u8(const float* src_nchw, uint8_t* dst_nhwc, int batch, int height, int width, void* hip_stream) {
  if (!src_nchw || !dst_nhwc || batch < 1 || height < 1 || width < 1) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_to_u8: bad arguments");
  const size_t total = (size_t)batch * height * width * 3;
  hipLaunchKernelGGL(swin_to_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), src_nchw,
                     dst_nhwc, height * width, total);
  HIPCHK(nullptr, hipGetLastError());
  return FDSR_OK;
}

}  // extern "C"
