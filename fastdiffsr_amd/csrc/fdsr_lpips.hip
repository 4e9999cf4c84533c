// LPIPS (AlexNet backbone, v0.1 linear heads) on uint8 images (gfx950): the fifth metric of the reference's val loop
// (FastDiffSR/core/metrics.py:154-163 calculate_lpips -> lpips.LPIPS(net='alex'); PerceptualSimilarity/networks_basic.py
// PNetLin.forward, pretrained_networks.py alexnet).
//
//   x      = ((u8 / 255) - shift) / scale               ToTensor() then ScalingLayer; the [0,1] image is NOT mapped to [-1,1]
//                                                        first (the reference does not pass normalize=True)
//   relu_k = the five ReLU outputs of torchvision AlexNet `features` (conv 11/4/2, pool, conv 5/1/2, pool, 3 x conv 3/1/1)
//   d_k    = mean over pixels of sum_c w_k[c] (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2
//   LPIPS  = d_0 + d_1 + d_2 + d_3 + d_4
//
// The convolutions are implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain per output), bias + ReLU
// in the epilogue; the 3/2 max-pools are a kernel of their own.  The truth image's features are computed once for the two
// test images (one batch of B * (1 + n_tests) forwards).  The distance runs in fp64 from the fp32 features, one wave per pixel,
// and the spatial mean is reduced in a fixed order (wave butterfly, waves in order, chunks in order): reruns are bitwise
// identical and an image's value depends neither on the batch size nor on its position in the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "fdsr_engine_int.h"

using namespace fdsr_int;

struct fdsr_lpips_obj {
  float* w[5] = {};      // conv weights packed [Kpad][Cout], k = (ky * KW + kx) * Cin + ci (NHWC gather order)
  float* b[5] = {};      // conv biases [Cout]
  float* lin[5] = {};    // linear heads [C]
};

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 64, BK = 16, NT = 256;
constexpr int AP = BM + 32;   // LDS row pitches: the two k rows an MFMA operand read touches sit 32 banks apart
constexpr int BP = BN + 32;
constexpr int DPIX = 64;      // pixels per distance workgroup (4 waves x 16, each wave in pixel order)

struct Layer { int cin, cout, k, s, p; };
constexpr Layer kLayers[5] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};
constexpr int kFeatIdx[5] = {0, 3, 6, 8, 10};   // torchvision alexnet.features indices of the five convolutions

struct ConvArgs {
  const float* x;                 // fp32 NHWC input (layers 1..4)
  const unsigned char* u8[3];     // layer 0: image set s = n / B (truth, test a, test b), each [B][Hin][Win][3]
  int B;
  const float* w;                 // [Kpad][Cout]
  const float* bias;
  float* out;                     // [N][Hout][Wout][Cout]
  int N, Hin, Win, Cin, Hout, Wout, Cout, KW, S, P, K, Kpad;
};

// One workgroup: BM output pixels x BN output channels; 4 waves in a 2 x 2 grid, each 64 pixels x 32 channels (two 32x32
// accumulators).  Thread t stages pixel t % BM and k-octet t / BM of every BK chunk (registers prefetch the next chunk while
// the MFMAs run on this one).  Out-of-image taps and k >= K read as zero (the zero padding of the SCALED tensor).
template <bool U8>
__global__ void __launch_bounds__(NT) lpips_conv_kernel(ConvArgs p) {
  __shared__ __attribute__((aligned(16))) float sA[BK * AP];
  __shared__ __attribute__((aligned(16))) float sB[BK * BP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int HWo = p.Hout * p.Wout;
  const int M = p.N * HWo;
  const int m0 = blockIdx.x * BM, co0 = blockIdx.y * BN;

  const int am = t & (BM - 1), ak = (t >> 7) * 8;
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
  const int bk = t >> 4, bn = (t & 15) * 4;

  float ra[8];
  f32x4 rb;
  auto load = [&](int kc) {
    const int kb = kc * BK;
    if (U8) {
      // ToTensor (x.float().div(255)) then ScalingLayer ((x - shift) / scale), IEEE division in torch's order
      const float shift[3] = {static_cast<float>(-.030), static_cast<float>(-.088), static_cast<float>(-.188)};
      const float scale[3] = {static_cast<float>(.458), static_cast<float>(.448), static_cast<float>(.450)};
      const unsigned char* img = p.u8[n / p.B] + (size_t)(n % p.B) * p.Hin * p.Win * 3;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = kb + ak + j;
        float v = 0.f;
        if (mval && k < p.K) {
          const int tap = k / 3, ci = k - 3 * tap;
          const int ky = tap / p.KW, kx = tap - ky * p.KW;
          const int iy = iy0 + ky, ix = ix0 + kx;
          if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) {
            const float x = __fdiv_rn((float)img[((size_t)iy * p.Win + ix) * 3 + ci], 255.0f);
            v = __fdiv_rn(__fsub_rn(x, shift[ci]), scale[ci]);
          }
        }
        ra[j] = v;
      }
    } else {
      // Cin % 8 == 0: the octet is 8 consecutive channels of one tap
      const int k = kb + ak;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
      if (mval && k < p.K) {
        const int tap = k / p.Cin, ci = k - tap * p.Cin;
        const int ky = tap / p.KW, kx = tap - ky * p.KW;
        const int iy = iy0 + ky, ix = ix0 + kx;
        if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) {
          const f32x4* src = reinterpret_cast<const f32x4*>(p.x + (((size_t)n * p.Hin + iy) * p.Win + ix) * p.Cin + ci);
          v0 = src[0];
          v1 = src[1];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { ra[j] = v0[j]; ra[4 + j] = v1[j]; }
    }
    rb = *reinterpret_cast<const f32x4*>(p.w + (size_t)(kb + bk) * p.Cout + co0 + bn);
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
      // 32x32x2 operands: A[i = lane & 31][k = lane >> 5] (pixel, k), B[k = lane >> 5][j = lane & 31] (k, channel)
      const int kr = 2 * s + h;
      const float bv = sB[kr * BP + wn * 32 + r31];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
        acc[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[kr * AP + wm * 64 + mb * 32 + r31], bv, acc[mb], 0, 0, 0);
    }
  }

  // epilogue: C/D map col = lane & 31 (channel), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (pixel); bias + ReLU
  const int co = co0 + wn * 32 + r31;
  const float bias = p.bias[co];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int om = m0 + wm * 64 + mb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (om < M) p.out[(size_t)om * p.Cout + co] = fmaxf(acc[mb][i] + bias, 0.f);
    }
}

// MaxPool2d(3, 2), floor mode, NHWC: every window lies inside the input (Hout = (Hin - 3) / 2 + 1)
__global__ void __launch_bounds__(256) lpips_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int Hin, int Win,
                                                            int C, int Ho, int Wo, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const size_t pix = i / C;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const size_t n = pix / ((size_t)Wo * Ho);
  float m = x[((n * Hin + 2 * oy) * Win + 2 * ox) * C + c];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, x[((n * Hin + 2 * oy + dy) * Win + 2 * ox + dx) * C + c]);
  y[i] = m;
}

__device__ __forceinline__ double wave_allsum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);   // partners add the same pair: every lane agrees
  return v;
}

// One layer's distance: workgroup = truth image n x a chunk of DPIX pixels; one wave per pixel (lane = channels c, c + 64, ...;
// C is 64, 192, 384 or 256).  part[((t * B + n) * 5 + layer) * maxch + chunk] = this chunk's sum of the per-pixel distances.
__global__ void __launch_bounds__(256) lpips_dist_kernel(const float* __restrict__ f, const float* __restrict__ lin, int B, int ntests,
                                                         int HW, int C, int chunks, int layer, int maxch, double* __restrict__ part) {
  __shared__ double red[2][4];
  const int chunk = blockIdx.x % chunks, n = blockIdx.x / chunks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpl = C / 64;
  double wl[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) wl[j] = j < cpl ? (double)lin[lane + 64 * j] : 0.0;
  double wsum[2] = {0.0, 0.0};
  for (int q = 0; q < DPIX / 4; ++q) {
    const int pix = chunk * DPIX + wave * (DPIX / 4) + q;
    if (pix >= HW) break;
    const float* f0 = f + ((size_t)n * HW + pix) * C;
    double a0[6], ss0 = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      a0[j] = j < cpl ? (double)f0[lane + 64 * j] : 0.0;
      ss0 += a0[j] * a0[j];
    }
    const double n0 = sqrt(wave_allsum(ss0)) + 1e-10;
    for (int tt = 0; tt < ntests; ++tt) {
      const float* f1 = f + ((size_t)((tt + 1) * B + n) * HW + pix) * C;
      double a1[6], ss1 = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        a1[j] = j < cpl ? (double)f1[lane + 64 * j] : 0.0;
        ss1 += a1[j] * a1[j];
      }
      const double n1 = sqrt(wave_allsum(ss1)) + 1e-10;
      double d = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double e = a0[j] / n0 - a1[j] / n1;
        d += wl[j] * (e * e);
      }
      wsum[tt] += wave_allsum(d);
    }
  }
  if (lane == 0) { red[0][wave] = wsum[0]; red[1][wave] = wsum[1]; }
  __syncthreads();
  if ((int)threadIdx.x < ntests) {
    const int tt = threadIdx.x;
    part[((size_t)(tt * B + n) * 5 + layer) * maxch + chunk] = ((red[tt][0] + red[tt][1]) + red[tt][2]) + red[tt][3];
  }
}

struct FinArgs { int chunks[5]; int hw[5]; };

// out[t][n][6] = (total, d_0 .. d_4): chunks summed in index order, / pixels, layers added 0..4 as PNetLin.forward does
__global__ void __launch_bounds__(64) lpips_finalize_kernel(const double* __restrict__ part, int B, int ntests, int maxch, FinArgs fa,
                                                            double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= ntests * B) return;
  double total = 0.0;
  for (int L = 0; L < 5; ++L) {
    double s = 0.0;
    for (int c = 0; c < fa.chunks[L]; ++c) s += part[((size_t)i * 5 + L) * maxch + c];
    const double v = s / (double)fa.hw[L];
    out[(size_t)i * 6 + 1 + L] = v;
    total = L == 0 ? v : total + v;
  }
  out[(size_t)i * 6] = total;
}

struct Plan {
  int ho[5], wo[5];      // conv output sizes
  int hp[2], wp[2];      // pool outputs (after layers 0 and 1)
  size_t off_f[5], off_p[2], off_part, bytes;
  int maxch;
};

int conv_out(int x, const Layer& l) { return (x + 2 * l.p - l.k) / l.s + 1; }

Plan make_plan(int B, int H, int W) {
  Plan pl{};
  const size_t NTI = (size_t)B * 3;   // truth + two tests
  int h = H, w = W;
  for (int L = 0; L < 5; ++L) {
    pl.ho[L] = conv_out(h, kLayers[L]);
    pl.wo[L] = conv_out(w, kLayers[L]);
    h = pl.ho[L];
    w = pl.wo[L];
    if (L < 2) {
      pl.hp[L] = (h - 3) / 2 + 1;
      pl.wp[L] = (w - 3) / 2 + 1;
      h = pl.hp[L];
      w = pl.wp[L];
    }
  }
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
  pl.maxch = 0;
  for (int L = 0; L < 5; ++L) {
    pl.off_f[L] = take(NTI * pl.ho[L] * pl.wo[L] * kLayers[L].cout * sizeof(float));
    if (L < 2) pl.off_p[L] = take(NTI * pl.hp[L] * pl.wp[L] * kLayers[L].cout * sizeof(float));
    pl.maxch = std::max(pl.maxch, (pl.ho[L] * pl.wo[L] + DPIX - 1) / DPIX);
  }
  pl.off_part = take((size_t)2 * B * 5 * pl.maxch * sizeof(double));
  pl.bytes = off;
  return pl;
}

int kpad(int L) { return round_up(kLayers[L].k * kLayers[L].k * kLayers[L].cin, BK); }

}  // namespace

extern "C" {

int fdsr_lpips_create(fdsr_lpips* out) {
  if (!out) return fail(nullptr, FDSR_E_INVALID, "fdsr_lpips_create: null output pointer");
  *out = new (std::nothrow) fdsr_lpips_obj();
  return *out ? FDSR_OK : fail(nullptr, FDSR_E_INVALID, "fdsr_lpips_create: out of host memory");
}

void fdsr_lpips_destroy(fdsr_lpips l) {
  if (!l) return;
  for (int L = 0; L < 5; ++L) {
    if (l->w[L]) (void)hipFree(l->w[L]);
    if (l->b[L]) (void)hipFree(l->b[L]);
    if (l->lin[L]) (void)hipFree(l->lin[L]);
  }
  delete l;
}

int fdsr_lpips_load(fdsr_lpips l, const char* name, const float* host_f32, const int64_t* shape, int ndim) {
  if (!l || !name || !host_f32 || (ndim > 0 && !shape) || ndim < 0)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_lpips_load: bad arguments");
  int layer = -1, kind = -1;   // kind 0: conv weight, 1: conv bias, 2: linear head
  for (int L = 0; L < 5 && layer < 0; ++L) {
    char buf[64];
    snprintf(buf, sizeof buf, "features.%d.weight", kFeatIdx[L]);
    if (!strcmp(name, buf)) { layer = L; kind = 0; break; }
    snprintf(buf, sizeof buf, "features.%d.bias", kFeatIdx[L]);
    if (!strcmp(name, buf)) { layer = L; kind = 1; break; }
    snprintf(buf, sizeof buf, "lin%d.model.1.weight", L);
    if (!strcmp(name, buf)) { layer = L; kind = 2; break; }
  }
  if (layer < 0) return fail(nullptr, FDSR_E_KEY, "fdsr_lpips_load: unknown tensor '%s'", name);
  const Layer& ly = kLayers[layer];
  std::vector<int64_t> want;
  if (kind == 0) want = {ly.cout, ly.cin, ly.k, ly.k};
  else if (kind == 1) want = {ly.cout};
  else want = {1, ly.cout, 1, 1};
  if (ndim != (int)want.size() || !std::equal(want.begin(), want.end(), shape))
    return fail(nullptr, FDSR_E_KEY, "fdsr_lpips_load: '%s' has the wrong shape", name);
  std::vector<float> host;
  float** dst;
  if (kind == 0) {   // [Cout][Cin][KH][KW] -> [Kpad][Cout], k = (ky * KW + kx) * Cin + ci; rows K..Kpad-1 zero
    host.assign((size_t)kpad(layer) * ly.cout, 0.f);
    for (int co = 0; co < ly.cout; ++co)
      for (int ci = 0; ci < ly.cin; ++ci)
        for (int ky = 0; ky < ly.k; ++ky)
          for (int kx = 0; kx < ly.k; ++kx)
            host[((size_t)(ky * ly.k + kx) * ly.cin + ci) * ly.cout + co] = host_f32[(((size_t)co * ly.cin + ci) * ly.k + ky) * ly.k + kx];
    dst = &l->w[layer];
  } else {
    host.assign(host_f32, host_f32 + ly.cout);
    dst = kind == 1 ? &l->b[layer] : &l->lin[layer];
  }
  if (!*dst) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(dst), host.size() * sizeof(float)));
  HIPCHK(nullptr, hipMemcpy(*dst, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  return FDSR_OK;
}

int fdsr_lpips_workspace_bytes(fdsr_lpips l, int batch, int height, int width, size_t* bytes) {
  if (!l || !bytes || batch < 1) return fail(nullptr, FDSR_E_INVALID, "fdsr_lpips_workspace_bytes: bad arguments");
  if (height < 32 || width < 32) return fail(nullptr, FDSR_E_INVALID, "LPIPS needs H, W >= 32 (got %dx%d)", height, width);
  *bytes = make_plan(batch, height, width).bytes;
  return FDSR_OK;
}

int fdsr_lpips_u8(fdsr_lpips l, const uint8_t* truth_nhwc, const uint8_t* test_a_nhwc, const uint8_t* test_b_nhwc, int batch,
                  int height, int width, double* out_dev, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!l || !truth_nhwc || !test_a_nhwc || !out_dev || !workspace || batch < 1)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_lpips_u8: bad arguments");
  if (height < 32 || width < 32) return fail(nullptr, FDSR_E_INVALID, "LPIPS needs H, W >= 32 (got %dx%d)", height, width);
  for (int L = 0; L < 5; ++L)
    if (!l->w[L] || !l->b[L] || !l->lin[L])
      return fail(nullptr, FDSR_E_STATE, "fdsr_lpips_u8: layer %d is missing a tensor (features.%d.weight / .bias, lin%d.model.1.weight)",
                  L, kFeatIdx[L], L);
  const Plan pl = make_plan(batch, height, width);
  if (workspace_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255))
    return fail(nullptr, FDSR_E_WORKSPACE, "fdsr_lpips_u8: workspace too small (%zu < %zu bytes) or not 256-byte aligned",
                workspace_bytes, pl.bytes);
  const int ntests = test_b_nhwc ? 2 : 1;
  const int N = batch * (1 + ntests);
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  char* ws = static_cast<char*>(workspace);
  const float* x = nullptr;
  int hin = height, win = width;
  for (int L = 0; L < 5; ++L) {
    const Layer& ly = kLayers[L];
    ConvArgs a{};
    a.x = x;
    a.u8[0] = truth_nhwc;
    a.u8[1] = test_a_nhwc;
    a.u8[2] = test_b_nhwc;
    a.B = batch;
    a.w = l->w[L];
    a.bias = l->b[L];
    a.out = reinterpret_cast<float*>(ws + pl.off_f[L]);
    a.N = N;
    a.Hin = hin;
    a.Win = win;
    a.Cin = ly.cin;
    a.Hout = pl.ho[L];
    a.Wout = pl.wo[L];
    a.Cout = ly.cout;
    a.KW = ly.k;
    a.S = ly.s;
    a.P = ly.p;
    a.K = ly.k * ly.k * ly.cin;
    a.Kpad = kpad(L);
    const int M = N * pl.ho[L] * pl.wo[L];
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(ly.cout / BN));
    if (L == 0) hipLaunchKernelGGL(lpips_conv_kernel<true>, grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(lpips_conv_kernel<false>, grid, dim3(NT), 0, st, a);
    HIPCHK(nullptr, hipGetLastError());
    x = a.out;
    hin = pl.ho[L];
    win = pl.wo[L];
    if (L < 2) {
      float* y = reinterpret_cast<float*>(ws + pl.off_p[L]);
      const size_t total = (size_t)N * pl.hp[L] * pl.wp[L] * ly.cout;
      hipLaunchKernelGGL(lpips_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, y, hin, win, ly.cout,
                         pl.hp[L], pl.wp[L], total);
      HIPCHK(nullptr, hipGetLastError());
      x = y;
      hin = pl.hp[L];
      win = pl.wp[L];
    }
  }
  double* part = reinterpret_cast<double*>(ws + pl.off_part);
  FinArgs fa{};
  for (int L = 0; L < 5; ++L) {
    const int hw = pl.ho[L] * pl.wo[L];
    fa.hw[L] = hw;
    fa.chunks[L] = (hw + DPIX - 1) / DPIX;
    hipLaunchKernelGGL(lpips_dist_kernel, dim3((unsigned)(batch * fa.chunks[L])), dim3(256), 0, st,
                       reinterpret_cast<const float*>(ws + pl.off_f[L]), l->lin[L], batch, ntests, hw, kLayers[L].cout, fa.chunks[L], L,
                       pl.maxch, part);
    HIPCHK(nullptr, hipGetLastError());
  }
  hipLaunchKernelGGL(lpips_finalize_kernel, dim3((unsigned)((ntests * batch + 63) / 64)), dim3(64), 0, st, part, batch, ntests, pl.maxch,
                     fa, out_dev);
  HIPCHK(nullptr, hipGetLastError());
  return FDSR_OK;
}

}  // extern "C"
