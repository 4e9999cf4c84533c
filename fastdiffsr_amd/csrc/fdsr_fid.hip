// FID features (pytorch_fid's InceptionV3, output_blocks=[3], resize_input=True, normalize_input=True, use_fid_inception=True) of
// uint8 images on gfx950: the network FastDiffSR/FID.py scores with (pytorch_fid.fid_score.calculate_fid_given_paths, dims=2048).
//
//   x     = 2 * bilinear_299(u8 / 255) - 1          ToTensor, F.interpolate(align_corners=False) -- every size, 299 included
//   conv  = BasicConv2d: conv (no bias) -> BatchNorm2d(eps=1e-3, eval) -> ReLU; the BN is folded into the conv on the host (fp64)
//   Conv2d_1a .. Conv2d_4a, two 3/2 max-pools, Mixed_5b .. Mixed_7c (FIDInceptionA / B / FIDInceptionC / D / FIDInceptionE_1,2)
//   pool3 = the global average of Mixed_7c: [B][2048]
//
// Every convolution (94 of them, seven kernel shapes, stride 1 and 2) is one implicit-GEMM kernel on v_mfma_f32_32x32x2_f32 (exact
// fp32: a k-ordered fmaf chain per output, no split-K), folded bias + ReLU in the epilogue, its output written at a channel
// offset / stride of the module's NHWC output so that the branch concatenations cost nothing.  Pools are kernels of their own;
// the global average is one thread per (image, channel) summing the pixels in order.  Every output element has one fixed
// summation order: reruns are bitwise identical and an image's features depend neither on B nor on its position in the batch.
//
// The network is written once, as a walk (Walker below) over named layers: the same code lists the 470 checkpoint tensors in
// load order, sizes the workspace and launches the kernels.
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
constexpr int RES = 299;      // pytorch_fid resizes every input to 299 x 299
constexpr int NMOD = 18;      // Conv2d_1a_3x3 .. Mixed_7c (include/fdsr.h lists the table)
constexpr int NBUF = 5;       // two module buffers (ping-pong) + three branch scratch buffers
constexpr char kBnSuffix[4][20] = {".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"};

struct LayerDesc {
  std::string name;             // e.g. "Mixed_5b.branch5x5_2"
  int cin, cout, kh, kw, s, ph, pw;
  int K() const { return kh * kw * cin; }
  int Kpad() const { return round_up(K(), BK); }
  int CoutPad() const { return round_up(cout, BN); }
};

struct ConvArgs {
  const float* x;               // fp32 NHWC input [N][Hin][Win][Cin]
  const float* w;               // [Kpad][CoutPad], k = (ky * KW + kx) * Cin + ci (NHWC gather order), BN folded
  const float* bias;            // [CoutPad], BN folded
  float* out;                   // [N][Hout][Wout][ostride], this conv's channels at [ooff, ooff + Cout)
  int N, Hin, Win, Cin, Hout, Wout, Cout, KW, S, PH, PW, K, Kpad, CoutPad, ooff, ostride;
};

// One workgroup: BM output pixels x BN output channels; 4 waves in a 2 x 2 grid, each 64 pixels x 32 channels (two 32x32
// accumulators).  Thread t stages pixel t % BM and k-octet t / BM of every BK chunk (registers prefetch the next chunk while the
// MFMAs run on this one).  Out-of-image taps and k >= K read as zero.  VEC: Cin % 8 == 0, the octet is 8 consecutive channels of
// one tap (every layer but Conv2d_1a_3x3, Cin = 3).
template <bool VEC>
__global__ void __launch_bounds__(NT) fid_conv_kernel(ConvArgs p) {
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
  const int iy0 = oy * p.S - p.PH, ix0 = ox * p.S - p.PW;
  const int bk = t >> 4, bn = (t & 15) * 4;

  float ra[8];
  f32x4 rb;
  auto load = [&](int kc) {
    const int kb = kc * BK;
    if (!VEC) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = kb + ak + j;
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
    rb = *reinterpret_cast<const f32x4*>(p.w + (size_t)(kb + bk) * p.CoutPad + co0 + bn);   // rows < Kpad, columns < CoutPad
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

  // epilogue: C/D map col = lane & 31 (channel), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (pixel); folded bias + ReLU, written
  // into the concatenated output at channel ooff + co
  const int co = co0 + wn * 32 + r31;
  if (co >= p.Cout) return;
  const float bias = p.bias[co];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int om = m0 + wm * 64 + mb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (om < M) p.out[(size_t)om * p.ostride + p.ooff + co] = fmaxf(acc[mb][i] + bias, 0.f);
    }
}

// u8 [B][H][W][3] -> fp32 [B][299][299][3]: ToTensor (a true division by 255), F.interpolate(size=(299, 299), mode='bilinear',
// align_corners=False) as torch's generic CPU kernel evaluates it (source index scale * (d + 0.5) - 0.5 clamped at 0, scale =
// float(in) / 299; the two taps of each row first, then the two rows), then 2x - 1.  Rounded operations, no contraction.
__global__ void __launch_bounds__(256) fid_stem_kernel(const unsigned char* __restrict__ img, float* __restrict__ y, int Hin, int Win,
                                                       size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % RES), oy = (int)((i / RES) % RES);
  const size_t n = i / ((size_t)RES * RES);
  auto index = [](int in, int d, int& i0, int& i1, float& l0, float& l1) {
    const float scale = __fdiv_rn((float)in, (float)RES);
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)d, 0.5f)), 0.5f);
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    l1 = fminf(__fsub_rn(src, (float)i0), 1.f);
    l0 = __fsub_rn(1.f, l1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
  };
  int y0, y1, x0, x1;
  float hy0, hy1, wx0, wx1;
  index(Hin, oy, y0, y1, hy0, hy1);
  index(Win, ox, x0, x1, wx0, wx1);
  const unsigned char* src = img + n * Hin * Win * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = __fdiv_rn((float)src[((size_t)y0 * Win + x0) * 3 + c], 255.f);
    const float b = __fdiv_rn((float)src[((size_t)y0 * Win + x1) * 3 + c], 255.f);
    const float d = __fdiv_rn((float)src[((size_t)y1 * Win + x0) * 3 + c], 255.f);
    const float e = __fdiv_rn((float)src[((size_t)y1 * Win + x1) * 3 + c], 255.f);
    const float t0 = __fadd_rn(__fmul_rn(a, wx0), __fmul_rn(b, wx1));
    const float t1 = __fadd_rn(__fmul_rn(d, wx0), __fmul_rn(e, wx1));
    const float v = __fadd_rn(__fmul_rn(t0, hy0), __fmul_rn(t1, hy1));
    y[i * 3 + c] = __fsub_rn(__fmul_rn(2.f, v), 1.f);
  }
}

enum PoolKind { MAX3S2 = 0, AVG3S1P1 = 1, MAX3S1P1 = 2 };

// NHWC pools, one thread per output element, taps in (dy, dx) order.  MAX3S2: MaxPool2d(3, 2), floor mode, every window inside
// the input.  AVG3S1P1: avg_pool2d(3, 1, 1, count_include_pad=False) -- the sum of the valid taps / their count.  MAX3S1P1:
// max_pool2d(3, 1, 1) (FIDInceptionE_2's branch_pool), the padding never wins.  Output at channel ooff of an ostride-wide tensor.
__global__ void __launch_bounds__(256) fid_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int kind, int Hin, int Win, int C,
                                                       int Ho, int Wo, int ooff, int ostride, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const size_t pix = i / C;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const size_t n = pix / ((size_t)Wo * Ho);
  const int s = kind == MAX3S2 ? 2 : 1, pad = kind == MAX3S2 ? 0 : 1;
  const bool avg = kind == AVG3S1P1;
  float acc = avg ? 0.f : -INFINITY;
  int cnt = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int iy = oy * s - pad + dy, ix = ox * s - pad + dx;
      if (iy < 0 || iy >= Hin || ix < 0 || ix >= Win) continue;
      const float v = x[((n * Hin + iy) * Win + ix) * C + c];
      acc = avg ? __fadd_rn(acc, v) : fmaxf(acc, v);
      ++cnt;
    }
  y[pix * ostride + ooff + c] = avg ? __fdiv_rn(acc, (float)cnt) : acc;
}

// adaptive_avg_pool2d(x, (1, 1)): out[n][c] = (sum of the HW pixels in order) / HW
__global__ void __launch_bounds__(256) fid_gap_kernel(const float* __restrict__ x, float* __restrict__ out, int HW, int C, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = i % C, n = i / C;
  float s = 0.f;
  for (int q = 0; q < HW; ++q) s = __fadd_rn(s, x[((size_t)n * HW + q) * C + c]);
  out[i] = __fdiv_rn(s, (float)HW);
}

// A view of a workspace buffer: [N][H][W][ctot], this tensor's channels at [coff, coff + C)
struct T { int buf, H, W, C, coff, ctot; };

enum Mode { TABLE, SIZE, RUN };

struct Walker {
  Mode mode;
  std::vector<LayerDesc>* table = nullptr;      // TABLE: appended to
  const std::vector<LayerDesc>* layers = nullptr;
  size_t need[NBUF] = {};                       // SIZE: floats per image of each buffer
  int N = 0, Hin = 0, Win = 0;
  const unsigned char* img = nullptr;
  float* buf[NBUF] = {};
  float* const* w = nullptr;
  float* const* b = nullptr;
  hipStream_t st = nullptr;
  int li = 0;                                   // the next layer's index (load order)
  int stop = NMOD;                              // RUN: the modules < stop (0: the stem only)
  int err = FDSR_OK;

  void touch(const T& t) { need[t.buf] = std::max(need[t.buf], (size_t)t.H * t.W * t.ctot); }

  void check(hipError_t e) {
    if (e != hipSuccess && err == FDSR_OK) err = fail(nullptr, FDSR_E_HIP, "fdsr_fid: kernel launch failed: %s", hipGetErrorString(e));
  }

  // out: the destination's buffer / channel offset / width (0: this conv's own Cout); its H, W, C are filled in here
  T conv(const std::string& name, const T& in, int cout, int kh, int kw, int s, int ph, int pw, T out) {
    out.H = (in.H + 2 * ph - kh) / s + 1;
    out.W = (in.W + 2 * pw - kw) / s + 1;
    out.C = cout;
    if (out.ctot == 0) out.ctot = cout;
    const int idx = li++;
    if (mode == TABLE) {
      table->push_back(LayerDesc{name, in.C, cout, kh, kw, s, ph, pw});
    } else if (mode == SIZE) {
      touch(out);
    } else if (err == FDSR_OK) {
      const LayerDesc& L = (*layers)[idx];
      ConvArgs a{};
      a.x = buf[in.buf];
      a.w = w[idx];
      a.bias = b[idx];
      a.out = buf[out.buf];
      a.N = N;
      a.Hin = in.H;
      a.Win = in.W;
      a.Cin = in.C;
      a.Hout = out.H;
      a.Wout = out.W;
      a.Cout = cout;
      a.KW = kw;
      a.S = s;
      a.PH = ph;
      a.PW = pw;
      a.K = L.K();
      a.Kpad = L.Kpad();
      a.CoutPad = L.CoutPad();
      a.ooff = out.coff;
      a.ostride = out.ctot;
      const int M = N * out.H * out.W;
      const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(L.CoutPad() / BN));
      if (in.C % 8 == 0) hipLaunchKernelGGL(fid_conv_kernel<true>, grid, dim3(NT), 0, st, a);
      else hipLaunchKernelGGL(fid_conv_kernel<false>, grid, dim3(NT), 0, st, a);
      check(hipGetLastError());
    }
    return out;
  }

  T pool(int kind, const T& in, T out) {
    out.H = kind == MAX3S2 ? (in.H - 3) / 2 + 1 : in.H;
    out.W = kind == MAX3S2 ? (in.W - 3) / 2 + 1 : in.W;
    out.C = in.C;
    if (out.ctot == 0) out.ctot = in.C;
    if (mode == SIZE) {
      touch(out);
    } else if (mode == RUN && err == FDSR_OK) {
      const size_t total = (size_t)N * out.H * out.W * out.C;
      hipLaunchKernelGGL(fid_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, buf[in.buf], buf[out.buf], kind, in.H,
                         in.W, in.C, out.H, out.W, out.coff, out.ctot, total);
      check(hipGetLastError());
    }
    return out;
  }

  static T at(int buf, int coff = 0, int ctot = 0) { return T{buf, 0, 0, 0, coff, ctot}; }

  // Modules (pytorch_fid/inception.py): `in` is a whole tensor, the output goes to buffer `ob`; scratch buffers 2, 3, 4.
  // Branch outputs land at their concatenation offsets, in torch.cat order.
  T inception_a(const std::string& m, const T& in, int pool_features, int ob) {
    const int ct = 64 + 64 + 96 + pool_features;
    T o = conv(m + ".branch1x1", in, 64, 1, 1, 1, 0, 0, at(ob, 0, ct));
    T t = conv(m + ".branch5x5_1", in, 48, 1, 1, 1, 0, 0, at(2));
    conv(m + ".branch5x5_2", t, 64, 5, 5, 1, 2, 2, at(ob, 64, ct));
    t = conv(m + ".branch3x3dbl_1", in, 64, 1, 1, 1, 0, 0, at(2));
    t = conv(m + ".branch3x3dbl_2", t, 96, 3, 3, 1, 1, 1, at(3));
    conv(m + ".branch3x3dbl_3", t, 96, 3, 3, 1, 1, 1, at(ob, 128, ct));
    t = pool(AVG3S1P1, in, at(4));
    conv(m + ".branch_pool", t, pool_features, 1, 1, 1, 0, 0, at(ob, 224, ct));
    return T{ob, o.H, o.W, ct, 0, ct};
  }

  T inception_b(const std::string& m, const T& in, int ob) {
    const int ct = 384 + 96 + in.C;
    T o = conv(m + ".branch3x3", in, 384, 3, 3, 2, 0, 0, at(ob, 0, ct));
    T t = conv(m + ".branch3x3dbl_1", in, 64, 1, 1, 1, 0, 0, at(2));
    t = conv(m + ".branch3x3dbl_2", t, 96, 3, 3, 1, 1, 1, at(3));
    conv(m + ".branch3x3dbl_3", t, 96, 3, 3, 2, 0, 0, at(ob, 384, ct));
    pool(MAX3S2, in, at(ob, 480, ct));
    return T{ob, o.H, o.W, ct, 0, ct};
  }

  T inception_c(const std::string& m, const T& in, int c7, int ob) {
    const int ct = 4 * 192;
    T o = conv(m + ".branch1x1", in, 192, 1, 1, 1, 0, 0, at(ob, 0, ct));
    T t = conv(m + ".branch7x7_1", in, c7, 1, 1, 1, 0, 0, at(2));
    t = conv(m + ".branch7x7_2", t, c7, 1, 7, 1, 0, 3, at(3));
    conv(m + ".branch7x7_3", t, 192, 7, 1, 1, 3, 0, at(ob, 192, ct));
    t = conv(m + ".branch7x7dbl_1", in, c7, 1, 1, 1, 0, 0, at(2));
    t = conv(m + ".branch7x7dbl_2", t, c7, 7, 1, 1, 3, 0, at(3));
    t = conv(m + ".branch7x7dbl_3", t, c7, 1, 7, 1, 0, 3, at(2));
    t = conv(m + ".branch7x7dbl_4", t, c7, 7, 1, 1, 3, 0, at(3));
    conv(m + ".branch7x7dbl_5", t, 192, 1, 7, 1, 0, 3, at(ob, 384, ct));
    t = pool(AVG3S1P1, in, at(4));
    conv(m + ".branch_pool", t, 192, 1, 1, 1, 0, 0, at(ob, 576, ct));
    return T{ob, o.H, o.W, ct, 0, ct};
  }

  T inception_d(const std::string& m, const T& in, int ob) {
    const int ct = 320 + 192 + in.C;
    T t = conv(m + ".branch3x3_1", in, 192, 1, 1, 1, 0, 0, at(2));
    T o = conv(m + ".branch3x3_2", t, 320, 3, 3, 2, 0, 0, at(ob, 0, ct));
    t = conv(m + ".branch7x7x3_1", in, 192, 1, 1, 1, 0, 0, at(2));
    t = conv(m + ".branch7x7x3_2", t, 192, 1, 7, 1, 0, 3, at(3));
    t = conv(m + ".branch7x7x3_3", t, 192, 7, 1, 1, 3, 0, at(2));
    conv(m + ".branch7x7x3_4", t, 192, 3, 3, 2, 0, 0, at(ob, 320, ct));
    pool(MAX3S2, in, at(ob, 512, ct));
    return T{ob, o.H, o.W, ct, 0, ct};
  }

  T inception_e(const std::string& m, const T& in, bool max_pool, int ob) {
    const int ct = 320 + 768 + 768 + 192;
    T o = conv(m + ".branch1x1", in, 320, 1, 1, 1, 0, 0, at(ob, 0, ct));
    T t = conv(m + ".branch3x3_1", in, 384, 1, 1, 1, 0, 0, at(2));
    conv(m + ".branch3x3_2a", t, 384, 1, 3, 1, 0, 1, at(ob, 320, ct));
    conv(m + ".branch3x3_2b", t, 384, 3, 1, 1, 1, 0, at(ob, 704, ct));
    t = conv(m + ".branch3x3dbl_1", in, 448, 1, 1, 1, 0, 0, at(3));
    t = conv(m + ".branch3x3dbl_2", t, 384, 3, 3, 1, 1, 1, at(4));
    conv(m + ".branch3x3dbl_3a", t, 384, 1, 3, 1, 0, 1, at(ob, 1088, ct));
    conv(m + ".branch3x3dbl_3b", t, 384, 3, 1, 1, 1, 0, at(ob, 1472, ct));
    t = pool(max_pool ? MAX3S1P1 : AVG3S1P1, in, at(2));
    conv(m + ".branch_pool", t, 192, 1, 1, 1, 0, 0, at(ob, 1856, ct));
    return T{ob, o.H, o.W, ct, 0, ct};
  }

  // The whole network.  The stem's output is in buffer 1, module k's in buffer k % 2.  Returns the last tensor computed.
  T walk() {
    T x{1, RES, RES, 3, 0, 3};
    if (mode == SIZE) {
      touch(x);
    } else if (mode == RUN && err == FDSR_OK) {
      const size_t total = (size_t)N * RES * RES;
      hipLaunchKernelGGL(fid_stem_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, img, buf[1], Hin, Win, total);
      check(hipGetLastError());
    }
    int k = 0;
    auto more = [&](T y) { x = y; ++k; return mode != RUN || k < stop; };
    if (mode == RUN && stop == 0) return x;
    if (!more(conv("Conv2d_1a_3x3", x, 32, 3, 3, 2, 0, 0, at(0)))) return x;
    if (!more(conv("Conv2d_2a_3x3", x, 32, 3, 3, 1, 0, 0, at(1)))) return x;
    if (!more(conv("Conv2d_2b_3x3", x, 64, 3, 3, 1, 1, 1, at(0)))) return x;
    if (!more(pool(MAX3S2, x, at(1)))) return x;
    if (!more(conv("Conv2d_3b_1x1", x, 80, 1, 1, 1, 0, 0, at(0)))) return x;
    if (!more(conv("Conv2d_4a_3x3", x, 192, 3, 3, 1, 0, 0, at(1)))) return x;
    if (!more(pool(MAX3S2, x, at(0)))) return x;
    if (!more(inception_a("Mixed_5b", x, 32, 1))) return x;
    if (!more(inception_a("Mixed_5c", x, 64, 0))) return x;
    if (!more(inception_a("Mixed_5d", x, 64, 1))) return x;
    if (!more(inception_b("Mixed_6a", x, 0))) return x;
    if (!more(inception_c("Mixed_6b", x, 128, 1))) return x;
    if (!more(inception_c("Mixed_6c", x, 160, 0))) return x;
    if (!more(inception_c("Mixed_6d", x, 160, 1))) return x;
    if (!more(inception_c("Mixed_6e", x, 192, 0))) return x;
    if (!more(inception_d("Mixed_7a", x, 1))) return x;
    if (!more(inception_e("Mixed_7b", x, false, 0))) return x;
    more(inception_e("Mixed_7c", x, true, 1));
    return x;
  }
};

const std::vector<LayerDesc>& layer_table() {
  static const std::vector<LayerDesc> table = [] {
    std::vector<LayerDesc> t;
    Walker wk{TABLE};
    wk.table = &t;
    wk.walk();
    return t;
  }();
  return table;
}

struct Plan { size_t off[NBUF]; size_t bytes; };

Plan make_plan(int B) {
  Walker wk{SIZE};
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

}  // namespace

struct fdsr_fid_obj {
  std::vector<std::vector<float>> host;   // [layer * 5 + j]: j = 0 conv.weight, 1..4 bn weight / bias / running_mean / running_var
  std::vector<unsigned char> have;        // [layer * 5 + j]
  std::vector<float*> w, b;               // device: folded weights [Kpad][CoutPad], folded bias [CoutPad]
};

extern "C" {

int fdsr_fid_create(fdsr_fid* out) {
  if (!out) return fail(nullptr, FDSR_E_INVALID, "fdsr_fid_create: null output pointer");
  const size_t n = layer_table().size();
  fdsr_fid f = new (std::nothrow) fdsr_fid_obj();
  if (!f) return fail(nullptr, FDSR_E_INVALID, "fdsr_fid_create: out of host memory");
  f->host.resize(n * 5);
  f->have.assign(n * 5, 0);
  f->w.assign(n, nullptr);
  f->b.assign(n, nullptr);
  *out = f;
  return FDSR_OK;
}

void fdsr_fid_destroy(fdsr_fid f) {
  if (!f) return;
  for (float* p : f->w)
    if (p) (void)hipFree(p);
  for (float* p : f->b)
    if (p) (void)hipFree(p);
  delete f;
}

int fdsr_fid_load(fdsr_fid f, const char* name, const float* host_f32, const int64_t* shape, int ndim) {
  if (!f || !name || !host_f32 || (ndim > 0 && !shape) || ndim < 0) return fail(nullptr, FDSR_E_INVALID, "fdsr_fid_load: bad arguments");
  const std::vector<LayerDesc>& tab = layer_table();
  int layer = -1, j = -1;
  for (size_t L = 0; L < tab.size() && layer < 0; ++L) {
    const std::string& p = tab[L].name;
    if (strncmp(name, p.c_str(), p.size())) continue;
    const char* rest = name + p.size();
    if (!strcmp(rest, ".conv.weight")) { layer = (int)L; j = 0; break; }
    for (int q = 0; q < 4; ++q)
      if (!strcmp(rest, kBnSuffix[q])) { layer = (int)L; j = 1 + q; break; }
  }
  if (layer < 0) return fail(nullptr, FDSR_E_KEY, "fdsr_fid_load: unknown tensor '%s'", name);
  const LayerDesc& L = tab[layer];
  std::vector<int64_t> want;
  if (j == 0) want = {L.cout, L.cin, L.kh, L.kw};
  else want = {L.cout};
  if (ndim != (int)want.size() || !std::equal(want.begin(), want.end(), shape))
    return fail(nullptr, FDSR_E_KEY, "fdsr_fid_load: '%s' has the wrong shape", name);
  f->host[(size_t)layer * 5 + j].assign(host_f32, host_f32 + numel(want));
  f->have[(size_t)layer * 5 + j] = 1;
  for (int q = 0; q < 5; ++q)
    if (!f->have[(size_t)layer * 5 + q]) return FDSR_OK;
  // the layer's five tensors are all here: fold the BN in fp64 (w' = w g / sqrt(var + 1e-3), b' = beta - mean g / sqrt(var + 1e-3)),
  // round to fp32, pack [Kpad][CoutPad] (k = (ky * KW + kx) * Cin + ci); rows K..Kpad-1 and columns Cout..CoutPad-1 stay zero
  const std::vector<float>* h = &f->host[(size_t)layer * 5];
  const int Cp = L.CoutPad();
  std::vector<float> wp((size_t)L.Kpad() * Cp, 0.f), bp((size_t)Cp, 0.f);
  for (int co = 0; co < L.cout; ++co) {
    const double scale = (double)h[1][co] / std::sqrt((double)h[4][co] + 1e-3);
    bp[co] = (float)((double)h[2][co] - (double)h[3][co] * scale);
    for (int ci = 0; ci < L.cin; ++ci)
      for (int ky = 0; ky < L.kh; ++ky)
        for (int kx = 0; kx < L.kw; ++kx)
          wp[((size_t)(ky * L.kw + kx) * L.cin + ci) * Cp + co] =
              (float)((double)h[0][(((size_t)co * L.cin + ci) * L.kh + ky) * L.kw + kx] * scale);
  }
  if (!f->w[layer]) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&f->w[layer]), wp.size() * sizeof(float)));
  if (!f->b[layer]) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&f->b[layer]), bp.size() * sizeof(float)));
  HIPCHK(nullptr, hipMemcpy(f->w[layer], wp.data(), wp.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(nullptr, hipMemcpy(f->b[layer], bp.data(), bp.size() * sizeof(float), hipMemcpyHostToDevice));
  return FDSR_OK;
}

int fdsr_fid_workspace_bytes(fdsr_fid f, int batch, int height, int width, size_t* bytes) {
  if (!f || !bytes || batch < 1 || height < 1 || width < 1)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_fid_workspace_bytes: bad arguments (B %d, %dx%d)", batch, height, width);
  *bytes = make_plan(batch).bytes;
  return FDSR_OK;
}

int fdsr_fid_features_u8(fdsr_fid f, const uint8_t* img_nhwc, int batch, int height, int width, int module, float* out_dev,
                         void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!f || !img_nhwc || !out_dev || !workspace || batch < 1 || height < 1 || width < 1 || module < -2 || module >= NMOD)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_fid_features_u8: bad arguments (B %d, %dx%d, module %d)", batch, height, width, module);
  const std::vector<LayerDesc>& tab = layer_table();
  for (size_t L = 0; L < tab.size(); ++L)
    for (int q = 0; q < 5; ++q)
      if (!f->have[L * 5 + q])
        return fail(nullptr, FDSR_E_STATE, "fdsr_fid_features_u8: tensor '%s%s' is missing", tab[L].name.c_str(),
                    q == 0 ? ".conv.weight" : kBnSuffix[q - 1]);
  const Plan pl = make_plan(batch);
  if (workspace_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(workspace) & 255))
    return fail(nullptr, FDSR_E_WORKSPACE, "fdsr_fid_features_u8: workspace too small (%zu < %zu bytes) or not 256-byte aligned",
                workspace_bytes, pl.bytes);
  Walker wk{RUN};
  wk.layers = &tab;
  wk.N = batch;
  wk.Hin = height;
  wk.Win = width;
  wk.img = img_nhwc;
  for (int i = 0; i < NBUF; ++i) wk.buf[i] = reinterpret_cast<float*>(static_cast<char*>(workspace) + pl.off[i]);
  wk.w = f->w.data();
  wk.b = f->b.data();
  wk.st = reinterpret_cast<hipStream_t>(hip_stream);
  wk.stop = module == -1 ? NMOD : module == -2 ? 0 : module + 1;
  const T x = wk.walk();
  if (wk.err != FDSR_OK) return wk.err;
  if (module == -1) {
    const int total = batch * x.C;
    hipLaunchKernelGGL(fid_gap_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, wk.st, wk.buf[x.buf], out_dev, x.H * x.W,
                       x.C, total);
    HIPCHK(nullptr, hipGetLastError());
  } else {
    HIPCHK(nullptr, hipMemcpyAsync(out_dev, wk.buf[x.buf], (size_t)batch * x.H * x.W * x.C * sizeof(float), hipMemcpyDeviceToDevice,
                                   wk.st));
  }
  return FDSR_OK;
}

}  // extern "C"
