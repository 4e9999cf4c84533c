// HSENet (MSI_SR_model/model/hsenet.py: HSENET) inference in exact fp32 on gfx950.
//
//   x     = sub_mean(img)                            a general 3x3 matrix + bias, NCHW -> NHWC       hsenet_input_kernel
//   f     = head(x);   n_basic_modules x BasicModule;   + f;   tail: conv + PixelShuffle per stage, conv n -> 3;   add_mean
//   BasicModule(x)   = x + tail(HSEM(head(x))), head and tail two conv3x3 + ReLU each
//   HSEM(x)          = x + relu(conv(cross(xb, up(SSEM_down(down(x))))))            xb = SSEM_base(x)
//   SSEM(x)          = x + relu(conv(mb * sigmoid(AB.1(NonLocal(h)))))              h = relu(conv(x)), mb = two conv + ReLU of h
//   NonLocal(x)      = W(softmax(theta(x)^T phi(x)) g(x)) + x        one head of n_feats / 2 channels, logits UNSCALED
//   cross(x0, x1)    = the same with theta on x1 (queries), phi and g on x0 (keys, values), + x0
//   down / up        = F.interpolate(bilinear, align_corners=False): the mean of 2 x 2 pixels (an odd last row / column is
//                      dropped), and the read at max(0, (o + 0.5) in / out - 0.5) with the neighbour clamped to in - 1
//
// The 3x3 and 1x1 GEMMs are fdsr_swin_common.h's with three epilogues added here (ReLU, ReLU + residual, the gate
// m * sigmoid(.)).  New here:
//   hsenet_attn_kernel   one head of d <= 32 over every pixel: one workgroup per (image, 32 queries), k and v streamed through
//                        LDS in chunks of 128 keys in order (registers hold the next chunk while the MFMAs run on this one),
//                        LDS independent of N.  Two passes that both form S^T on the MFMA (score_tile): the first keeps the exact
//                        row maxima.  In the second a lane's 16 scores of a tile are, as they stand, the A operand of
//                        v_mfma_f32_32x32x2_f32 against v rows read in the same key order: exp(s - max) goes from the
//                        accumulator into P V without a trip through LDS.  Each wave sums its 32 keys of every chunk; the four
//                        waves' sums and row sums are added in wave order at the end; the quotient comes last.  No rescaling.
//   hsenet_down2_kernel, hsenet_up_kernel   the two resamplings on NHWC.
// Every output element has one fixed summation order: reruns are bitwise equal and an image's result depends neither on B nor
// on its place in the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fdsr_engine_int.h"
#include "fdsr_swin_common.h"
#include "fdsr_swin_engine.h"

using namespace fdsr_int;

namespace {

constexpr int VP = HD + 8;   // pitch of the [key][d] chunk: the two key rows an MFMA operand read touches (4 apart) sit 32 banks apart

enum HsenetEpi { EPI_RELU = EPI_EXT, EPI_RELU_RES = EPI_EXT + 1, EPI_GATE = EPI_EXT + 2 };

template <int EPI, class ARGS>
__device__ void gemm_epilogue_ext(const ARGS& p, const f32x16 (&acc)[2], int row0, int co, int h, float bias) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int om = acc_row(row0 + mb * 32, i, h);
      if (om >= p.M) continue;
      const float v = acc[mb][i] + bias;
      const size_t o = (size_t)om * p.N + co;
      if constexpr (EPI == EPI_RELU) {
        p.out[o] = fmaxf(v, 0.f);
      } else if constexpr (EPI == EPI_RELU_RES) {
        p.out[o] = p.res[o] + fmaxf(v, 0.f);   // res may be out
      } else {
        p.out[o] = p.res[o] * (1.f / (1.f + expf(-v)));   // EPI_GATE: res is the main branch
      }
    }
}

// [B][3][H][W] -> NHWC [B][H][W][3], y = A x + b: sub_mean as the checkpoint holds it (A [3][3] row-major, out x in)
__global__ void __launch_bounds__(256) hsenet_input_kernel(const float* __restrict__ x, const float* __restrict__ A, const float* __restrict__ bias,
                                                           float* __restrict__ y, int HW, size_t pixels) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const size_t b = i / HW, pix = i - b * HW;
  const float* s = x + b * 3 * HW + pix;
  const float v0 = s[0], v1 = s[HW], v2 = s[2 * (size_t)HW];
#pragma unroll
  for (int c = 0; c < 3; ++c) y[i * 3 + c] = A[c * 3] * v0 + A[c * 3 + 1] * v1 + A[c * 3 + 2] * v2 + bias[c];
}

// NHWC [B][H][W][3] -> [B][3][H][W], y = A x + b: add_mean
__global__ void __launch_bounds__(256) hsenet_output_kernel(const float* __restrict__ x, const float* __restrict__ A, const float* __restrict__ bias,
                                                            float* __restrict__ y, int HW, size_t pixels) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const size_t b = i / HW, pix = i - b * HW;
  const float v0 = x[i * 3], v1 = x[i * 3 + 1], v2 = x[i * 3 + 2];
#pragma unroll
  for (int c = 0; c < 3; ++c) y[(b * 3 + c) * HW + pix] = A[c * 3] * v0 + A[c * 3 + 1] * v1 + A[c * 3 + 2] * v2 + bias[c];
}

// out = a + b over `quads` float4
__global__ void __launch_bounds__(256) hsenet_add_kernel(const f32x4* __restrict__ a, const f32x4* __restrict__ b, f32x4* __restrict__ out, size_t quads) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < quads) out[i] = a[i] + b[i];
}

// F.interpolate(scale_factor=0.5, bilinear, align_corners=False) on NHWC: [B][H][W][C] -> [B][H / 2][W / 2][C], the mean of pixels
// (2i, 2i + 1) x (2j, 2j + 1); C4 = C / 4
__global__ void __launch_bounds__(256) hsenet_down2_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ y, int H, int W, int C4, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int h = H / 2, w = W / 2;
  const int c = (int)(i % C4);
  const size_t pix = i / C4;
  const int ox = (int)(pix % w), oy = (int)((pix / w) % h);
  const size_t b = pix / ((size_t)w * h);
  const f32x4* r0 = x + ((b * H + 2 * oy) * W + 2 * ox) * C4 + c;
  const f32x4* r1 = r0 + (size_t)W * C4;
  y[i] = 0.5f * (0.5f * r0[0] + 0.5f * r0[C4]) + 0.5f * (0.5f * r1[0] + 0.5f * r1[C4]);
}

// F.interpolate(size=(H, W), bilinear, align_corners=False) on NHWC: [B][h][w][C] -> [B][H][W][C]
__global__ void __launch_bounds__(256) hsenet_up_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ y, int h, int w, int H, int W, int C4,
                                                        size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4);
  const size_t pix = i / C4;
  const int ox = (int)(pix % W), oy = (int)((pix / W) % H);
  const size_t b = pix / ((size_t)W * H);
  const float sy = fmaxf((float)h / (float)H * (oy + 0.5f) - 0.5f, 0.f), sx = fmaxf((float)w / (float)W * (ox + 0.5f) - 0.5f, 0.f);
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < h - 1), x1 = x0 + (x0 < w - 1);
  const float ly = sy - y0, lx = sx - x0;
  const f32x4* s = x + b * h * w * C4 + c;
  const f32x4 top = (1.f - lx) * s[((size_t)y0 * w + x0) * C4] + lx * s[((size_t)y0 * w + x1) * C4];
  const f32x4 bot = (1.f - lx) * s[((size_t)y1 * w + x0) * C4] + lx * s[((size_t)y1 * w + x1) * C4];
  y[i] = (1.f - ly) * top + ly * bot;
}

// Non-local attention of one (image, block of QB queries): O[i][c] = sum_j softmax_j(q_i . k_j) v[j][c], c < D <= 32, D % 4 == 0.
// q [B][Nq][D], k and v [B][Nk][D], out [B][Nq][D], rows contiguous.  Columns >= D are zeros in LDS.  Keys >= Nk of the last
// chunk are zero rows that enter neither the max nor the sum (their e is 0, as is their v); queries >= Nq are zero rows that are
// not stored.
__global__ void __launch_bounds__(256) hsenet_attn_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                          float* __restrict__ out, int D, int Nq, int Nk) {
  __shared__ __attribute__((aligned(16))) float sQt[HD * QB];   // [d][query]
  __shared__ __attribute__((aligned(16))) float sK[HD * KP];    // [d][key] of the chunk; at the end the four waves' O [wave][query][d]
  __shared__ __attribute__((aligned(16))) float sV[KC * VP];    // [key][d] of the chunk
  __shared__ float sRed[4 * QB];
  __shared__ float sM[QB];
  static_assert(4 * QB * HD <= HD * KP, "the waves' outputs fit the k chunk");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nqb = (Nq + QB - 1) / QB;
  const int qb = blockIdx.x % nqb, b = blockIdx.x / nqb;
  const int q0 = qb * QB;
  const int r31 = lane & 31, h = lane >> 5;
  const float* kb = k + (size_t)b * Nk * D;
  const float* vb = v + (size_t)b * Nk * D;

  {
    const int i = t & 31, d0 = (t >> 5) * 4;
    f32x4 qv = {0.f, 0.f, 0.f, 0.f};
    if (q0 + i < Nq && d0 < D) qv = *reinterpret_cast<const f32x4*>(q + ((size_t)b * Nq + q0 + i) * D + d0);
#pragma unroll
    for (int e = 0; e < 4; ++e) sQt[(d0 + e) * QB + i] = qv[e];
  }

  // thread t holds 16 columns of key row t % 128 of the next chunk, and four quads of its v rows
  const int kj = t & (KC - 1), kd0 = (t >> 7) * 16;
  f32x4 rk[4], rv[4];
  auto load_k = [&](int c0) {
    const bool ok = c0 + kj < Nk;
    const float* row = kb + (size_t)(ok ? c0 + kj : 0) * D + kd0;
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      rk[e4] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok && kd0 + 4 * e4 < D) rk[e4] = *reinterpret_cast<const f32x4*>(row + 4 * e4);
    }
  };
  auto store_k = [&]() {
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4)
#pragma unroll
      for (int e = 0; e < 4; ++e) sK[(kd0 + 4 * e4 + e) * KP + kj] = rk[e4][e];
  };
  auto load_v = [&](int c0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = t + 256 * e, jj = idx >> 3, d4 = (idx & 7) * 4;
      rv[e] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c0 + jj < Nk && d4 < D) rv[e] = *reinterpret_cast<const f32x4*>(vb + (size_t)(c0 + jj) * D + d4);
    }
  };
  auto store_v = [&]() {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = t + 256 * e, jj = idx >> 3, d4 = (idx & 7) * 4;
      *reinterpret_cast<f32x4*>(sV + jj * VP + d4) = rv[e];
    }
  };
  // St[j][i] of this wave's 32 keys of the chunk: row j = acc_row(32 wave, r, h), column i = r31
  auto scores = [&]() { return score_tile(sK, KP, wave * 32, sQt, QB, 0, r31, h); };

  // pass 1: the row maxima
  float m = -INFINITY;
  load_k(0);
  for (int c0 = 0; c0 < Nk; c0 += KC) {
    __syncthreads();   // the previous chunk's operand reads are done (first: sQt is written)
    store_k();
    __syncthreads();
    if (c0 + KC < Nk) load_k(c0 + KC);
    const f32x16 acc = scores();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = acc_row(c0 + wave * 32, r, h);
      if (j < Nk) m = fmaxf(m, acc[r]);
    }
  }
  load_k(0);
  load_v(0);
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (h == 0) sRed[wave * QB + r31] = m;
  __syncthreads();
  if (t < QB) sM[t] = fmaxf(fmaxf(sRed[t], sRed[QB + t]), fmaxf(sRed[2 * QB + t], sRed[3 * QB + t]));
  __syncthreads();
  m = sM[r31];

  // pass 2: e = exp(s - max), the row sums, O += e v.  32x32x2 operands: A[i = lane & 31][k = lane >> 5] (query, key),
  // B[k = lane >> 5][j = lane & 31] (key, d); step r takes key acc_row(32 wave, r, h) of half h for both.
  f32x16 o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  float lsum = 0.f;
  for (int c0 = 0; c0 < Nk; c0 += KC) {
    __syncthreads();   // the previous chunk's reads of sK and sV are done (first: sRed and sM are read)
    store_k();
    store_v();
    __syncthreads();
    if (c0 + KC < Nk) {
      load_k(c0 + KC);
      load_v(c0 + KC);
    }
    const f32x16 acc = scores();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jl = acc_row(wave * 32, r, h);
      const float e = c0 + jl < Nk ? expf(acc[r] - m) : 0.f;
      lsum += e;
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(e, sV[jl * VP + r31], o, 0, 0, 0);
    }
  }
  // the row sums: this lane's keys, the other half of the wave; then sums and outputs of the four waves in wave order
  lsum += __shfl_xor(lsum, 32, 64);
  __syncthreads();   // the last chunk's reads of sK are done
  if (h == 0) sRed[wave * QB + r31] = lsum;
  float* sO = sK;
#pragma unroll
  for (int i = 0; i < 16; ++i) sO[(wave * QB + acc_row(0, i, h)) * HD + r31] = o[i];
  __syncthreads();
  const int qi = t >> 3, d4 = (t & 7) * 4;
  if (q0 + qi < Nq && d4 < D) {
    const float l = ((sRed[qi] + sRed[QB + qi]) + sRed[2 * QB + qi]) + sRed[3 * QB + qi];
    const f32x4* po = reinterpret_cast<const f32x4*>(sO + qi * HD + d4);
    const f32x4 sum = ((po[0] + po[QB * HD / 4]) + po[2 * QB * HD / 4]) + po[3 * QB * HD / 4];
    *reinterpret_cast<f32x4*>(out + ((size_t)b * Nq + q0 + qi) * D + d4) = sum / l;
  }
}

enum Kind { CONV, CONV1, MEAN };

// One named module of the checkpoint: name.weight and name.bias
struct LayerDesc {
  std::string name;
  Kind kind;
  int cin, cout;
  int tensors() const { return 2; }
  std::string tensor_name(int j) const { return name + (j == 0 ? ".weight" : ".bias"); }
  std::vector<int64_t> shape(int j) const {
    if (j == 1) return {cout};
    if (kind == CONV) return {cout, cin, 3, 3};
    return {cout, cin, 1, 1};
  }
};

struct Walker;

// what fdsr_swin_engine.h needs to know of this family
struct Hsenet : FamilyDefaults {
  using Config = fdsr_hsenet_config;
  using Desc = LayerDesc;
  using Walk = Walker;
  using Obj = fdsr_hsenet_obj;
  static constexpr const char *name = "fdsr_hsenet", *graph_flag_name = "FDSR_HSENET_GRAPH";
  static constexpr int NBUF = 21, SIDE = 8, graph_flag = FDSR_HSENET_GRAPH;

  static int check_shape(const char* fn, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, B, H, W);
    if (H < 2 || W < 2) return fail(nullptr, FDSR_E_INVALID, "%s: a %dx%d image has no half-scale pixel (both sides must be at least 2)", fn, H, W);
    if ((long long)B * H * W * 64 > (1ll << 30)) return fail(nullptr, FDSR_E_INVALID, "%s: %d images of %dx%d are too many pixels for one call", fn, B, H, W);
    return FDSR_OK;
  }

  // device: CONV / CONV1 packed [Kpad][Npad] + bias [Npad]; MEAN as the checkpoint holds it
  static void pack(const LayerDesc& L, int j, const float* host_f32, std::vector<float>& packed) {
    if (L.kind == MEAN) packed.assign(host_f32, host_f32 + (j == 1 ? 3 : 9));
    else pack_gemm_tensor(L.kind == CONV, j == 1, L.cin, L.cout, host_f32, packed);
  }
};

struct Walker : WalkerBase<Hsenet> {
  // out = epilogue(gather(in) . W + bias).  res: the addend of EPI_RES / EPI_RELU_RES (may be the output), the factor of EPI_GATE.
  // r: the EPI_SHUFFLE factor.
  T gemm(const std::string& name, Kind kind, int epi, const T& in, int cout, int ob, const T* res = nullptr, int r = 1) {
    const int idx = layer(name, kind, in.C, cout);
    const T out{ob, in.H * r, in.W * r, cout / (r * r)};
    if (mode == SIZE) touch(out);
    if (!live()) return out;
    GemmArgs a{};
    gemm_args(a, idx, in, res, kind == CONV, in.C, cout, r);
    a.out = buf[ob];
    const bool vec = in.C % 4 == 0;
    if (kind == CONV) {
      if (epi == EPI_NONE) check(launch_swin_gemm<CONV3, EPI_NONE>(a, vec, st));
      else if (epi == EPI_RELU) check(launch_swin_gemm<CONV3, EPI_RELU>(a, vec, st));
      else if (epi == EPI_RELU_RES) check(launch_swin_gemm<CONV3, EPI_RELU_RES>(a, vec, st));
      else check(launch_swin_gemm<CONV3, EPI_SHUFFLE>(a, vec, st));
    } else {
      if (epi == EPI_NONE) check(launch_swin_gemm<ROWS, EPI_NONE>(a, vec, st));
      else if (epi == EPI_RES) check(launch_swin_gemm<ROWS, EPI_RES>(a, vec, st));
      else check(launch_swin_gemm<ROWS, EPI_GATE>(a, vec, st));
    }
    return out;
  }

  void mean_shift(const char* name, bool input, const T& t) {
    const int idx = layer(name, MEAN, 3, 3);
    if (!live() || (!input && !dst)) return;
    const size_t pixels = (size_t)N * t.H * t.W;
    const dim3 grid((unsigned)((pixels + 255) / 256));
    if (input) hipLaunchKernelGGL(hsenet_input_kernel, grid, dim3(256), 0, st, img, w[idx], b[idx], buf[t.buf], t.H * t.W, pixels);
    else hipLaunchKernelGGL(hsenet_output_kernel, grid, dim3(256), 0, st, buf[t.buf], w[idx], b[idx], dst, t.H * t.W, pixels);
    check(hipGetLastError());
  }

  // the three elementwise kernels: out = a + b, the half-scale mean, the bilinear read at (H, W)
  T pointwise(int what, const T& in, const T* other, int H, int W, int ob) {
    const T out{ob, H, W, in.C};
    if (mode == SIZE) touch(out);
    if (!live()) return out;
    const int C4 = in.C / 4;
    const size_t total = (size_t)N * H * W * C4;
    const dim3 grid((unsigned)((total + 255) / 256));
    const f32x4* src = reinterpret_cast<const f32x4*>(buf[in.buf]);
    f32x4* o = reinterpret_cast<f32x4*>(buf[ob]);
    if (what == 0) hipLaunchKernelGGL(hsenet_add_kernel, grid, dim3(256), 0, st, src, reinterpret_cast<const f32x4*>(buf[other->buf]), o, total);
    else if (what == 1) hipLaunchKernelGGL(hsenet_down2_kernel, grid, dim3(256), 0, st, src, o, in.H, in.W, C4, total);
    else hipLaunchKernelGGL(hsenet_up_kernel, grid, dim3(256), 0, st, src, o, in.H, in.W, H, W, C4, total);
    check(hipGetLastError());
    return out;
  }

  // NonLocalBlock2D (x1 = x0) and AdjustedNonLocalBlock: W(softmax(theta(x1)^T phi(x0)) g(x0)) + x0; ob may be x0's buffer
  T nonlocal(const std::string& p, const T& x0, const T& x1, int ob) {
    const int ci = cfg.n_feats / 2;
    const T g = gemm(p + ".g", CONV1, EPI_NONE, x0, ci, 12);
    const T th = gemm(p + ".theta", CONV1, EPI_NONE, x1, ci, 10);
    const T ph = gemm(p + ".phi", CONV1, EPI_NONE, x0, ci, 11);
    const T y{13, x1.H, x1.W, ci};
    if (mode == SIZE) touch(y);
    if (live()) {
      const int Nq = x1.H * x1.W, Nk = x0.H * x0.W;
      const unsigned blocks = (unsigned)(N * ((Nq + QB - 1) / QB));
      hipLaunchKernelGGL(hsenet_attn_kernel, dim3(blocks), dim3(256), 0, st, buf[th.buf], buf[ph.buf], buf[g.buf], buf[13], ci, Nq, Nk);
      check(hipGetLastError());
    }
    return gemm(p + ".W", CONV1, EPI_RES, y, cfg.n_feats, ob, &x0);
  }

  // SSEM: buffers 7, 8, 9 (and the non-local block's 10 .. 13); ob is not s's buffer
  T ssem(const std::string& p, const std::string& tp, const T& s, int ob) {
    const int nf = cfg.n_feats;
    const T hh = gemm(p + ".head.0.0", CONV, EPI_RELU, s, nf, 7);
    const T m1 = gemm(p + ".MB.0.0", CONV, EPI_RELU, hh, nf, 8);
    const T m2 = gemm(p + ".MB.1.0", CONV, EPI_RELU, m1, nf, 9);
    const T z = nonlocal(p + ".AB.0", hh, hh, 8);
    tap(tp + ".nl", z);
    const T gate = gemm(p + ".AB.1", CONV1, EPI_GATE, z, nf, 7, &m2);
    tap(tp + ".gate", gate);
    const T out = gemm(p + ".tail.0.0", CONV, EPI_RELU_RES, gate, nf, ob, &s);
    tap(tp, out);
    return out;
  }

  // BasicModule: x -> ob.  Buffers: 4 the first head block, then the HSEM's output; 5 the HSEM's input; 6 the base SSEM's output,
  // then the first tail block; 14 / 15 the half-scale input and SSEM output; 16 its upsampled map; 17 the cross block's output
  T basic_module(const std::string& p, const std::string& tp, const T& x, int ob) {
    const int nf = cfg.n_feats;
    const T a = gemm(p + ".head.0.0", CONV, EPI_RELU, x, nf, 4);
    const T bb = gemm(p + ".head.1.0", CONV, EPI_RELU, a, nf, 5);
    tap(tp + ".head", bb);
    const std::string hp = p + ".body.0";
    const T xb = ssem(hp + ".base_scale.0", tp + ".base", bb, 6);
    const T d = pointwise(1, bb, nullptr, bb.H / 2, bb.W / 2, 14);
    tap(tp + ".down.in", d);
    const T xd = ssem(hp + ".down_scale.0", tp + ".down", d, 15);
    const T xu = pointwise(2, xd, nullptr, bb.H, bb.W, 16);
    tap(tp + ".up", xu);
    const T nl = nonlocal(hp + ".NonLocal_base", xb, xu, 17);
    tap(tp + ".cross", nl);
    const T hs = gemm(hp + ".tail.0.0", CONV, EPI_RELU_RES, nl, nf, 4, &bb);
    tap(tp + ".hsem", hs);
    const T t1 = gemm(p + ".tail.0.0", CONV, EPI_RELU, hs, nf, 6);
    const T out = gemm(p + ".tail.1.0", CONV, EPI_RELU_RES, t1, nf, ob, &x);
    tap(tp, out);
    return out;
  }

  // The whole network.  Buffers: 0 the input after sub_mean, 1 head's output, 2 / 3 the modules' outputs in turn, 4 .. 17 a
  // module's (above), 18 / 19 the upsampler's stages, 20 the last convolution's output.
  void walk() {
    const int nf = cfg.n_feats, H = std::max(Hin, 2), W = std::max(Win, 2);
    T x{0, H, W, 3};
    if (mode == SIZE) touch(x);
    mean_shift("sub_mean", true, x);
    const T f = gemm("head.0", CONV, EPI_NONE, x, nf, 1);
    tap("head", f);
    T cur = f;
    for (int i = 0; i < cfg.n_basic_modules; ++i)
      cur = basic_module("body_modulist." + std::to_string(i), "m" + std::to_string(i), cur, cur.buf == 2 ? 3 : 2);
    T u = pointwise(0, cur, &f, H, W, cur.buf == 2 ? 3 : 2);
    tap("body", u);
    if (cfg.scale == 3) {
      u = gemm("tail.0.0", CONV, EPI_SHUFFLE, u, 9 * nf, 18, nullptr, 3);
    } else {
      for (int k = 0; (1 << k) < cfg.scale; ++k) u = gemm("tail.0." + std::to_string(2 * k), CONV, EPI_SHUFFLE, u, 4 * nf, u.buf == 18 ? 19 : 18, nullptr, 2);
    }
    tap("up", u);
    const T tl = gemm("tail.1", CONV, EPI_NONE, u, 3, 20);
    mean_shift("add_mean", false, tl);
  }
};

}  // namespace

struct fdsr_hsenet_obj : Engine<Hsenet> {};

extern "C" {

int fdsr_hsenet_create(const fdsr_hsenet_config* cfg, fdsr_hsenet* out) {
  if (!cfg || !out) return fail(nullptr, FDSR_E_INVALID, "fdsr_hsenet_create: null argument");
  const fdsr_hsenet_config& c = *cfg;
  if (c.n_colors != 3) return fail(nullptr, FDSR_E_INVALID, "fdsr_hsenet_create: n_colors %d is not supported (3 only)", c.n_colors);
  if (c.n_feats != 16 && c.n_feats != 32 && c.n_feats != 64)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_hsenet_create: n_feats %d is not supported (16, 32, 64: one head of n_feats / 2 <= 32)", c.n_feats);
  if (c.scale != 2 && c.scale != 3 && c.scale != 4 && c.scale != 8)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_hsenet_create: scale %d is not supported (2, 3, 4, 8)", c.scale);
  if (c.n_basic_modules < 1) return fail(nullptr, FDSR_E_INVALID, "fdsr_hsenet_create: n_basic_modules %d (at least 1)", c.n_basic_modules);
  return engine_create<Hsenet>("fdsr_hsenet_create", c, out);
}

void fdsr_hsenet_destroy(fdsr_hsenet s) { engine_destroy<Hsenet>(s); }

int fdsr_hsenet_load(fdsr_hsenet s, const char* name, const float* host_f32, const int64_t* shape, int ndim) {
  return engine_load<Hsenet>("fdsr_hsenet_load", s, name, host_f32, shape, ndim);
}

int fdsr_hsenet_workspace_bytes(fdsr_hsenet s, int batch, int height, int width, size_t* bytes) {
  return engine_workspace_bytes<Hsenet>("fdsr_hsenet_workspace_bytes", s, batch, height, width, bytes);
}

int fdsr_hsenet_forward(fdsr_hsenet s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace,
                        size_t workspace_bytes, void* hip_stream, int flags) {
  return engine_forward<Hsenet>("fdsr_hsenet_forward", s, x_nchw, batch, height, width, out_nchw, workspace, workspace_bytes, hip_stream, flags);
}

int fdsr_hsenet_debug_tensor(fdsr_hsenet s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                             size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return engine_debug_tensor<Hsenet>("fdsr_hsenet_debug_tensor", s, name, x_nchw, batch, height, width, out_nhwc, capacity_floats, dims3,
                                     workspace, workspace_bytes, hip_stream);
}

}  // extern "C"
