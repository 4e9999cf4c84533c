// gfx950 (MI355X / CDNA4) kernels of the FastDiffSR sampling path.
//
// Layout: every activation is NHWC fp32 in HBM.  The convolutions are implicit
// GEMMs on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32
// (M = 32 output pixels, N = 32 output channels, K = 2 input channels per issue):
//   * one 256-thread workgroup = 4 wave64 = an 8x16 output-pixel tile x BN channels
//   * per K-chunk (KC input channels) the input halo tile is staged ONCE into LDS
//     -- GroupNorm-apply + Swish fused into that staging (unet.py:89-101) -- and
//     reused by all 9 taps; the weight slab [tap][BN][KC] is staged next to it
//   * LDS rows are KC+4 floats: 16-byte aligned for ds_write_b128 / ds_read_b128
//     and (KC+4)/4 odd, so the 16 lanes of a ds_read_b128 group hit 16 distinct
//     16-byte slots (conflict-free); each lane reads 4 consecutive k of its
//     pixel row at once and feeds 4 MFMAs from it
//   * global loads of chunk k+1 are issued before the MFMAs of chunk k (register
//     prefetch), 2 workgroups per CU cover each other's staging phases
//   * epilogue: + bias + per-sample noise-embedding shift (unet.py:38-54) +
//     residual, stored NHWC (each lane owns one output channel: 128-B segments)
// Everything else on the path (GroupNorm statistics, CLAM/SLAM, the posterior
// update, layout changes at the boundary) is HBM-bound streaming code.
#include "fdsr_conv_dev.h"
#include "fdsr_philox.h"

#include <string>

namespace fdsr {

// ---------------------------------------------------------------------------
// convolution
// ---------------------------------------------------------------------------
template <int KS, int STRIDE, bool UP, int KC, int BN, int WM>
struct ConvCfg {
  static constexpr int TH = 8, TW = 16;
  static constexpr int PAD = KS / 2;
  static constexpr int HH = (TH - 1) * STRIDE + KS;
  static constexpr int HWD = (TW - 1) * STRIDE + KS;
  static constexpr int NPIX = HH * HWD;
  static constexpr int S = KC + 4;
  static constexpr int Q = KC / 4;
  static constexpr int RPP = 256 / Q;  // LDS rows covered per pass of the 256 threads
  static constexpr int NIN = (NPIX + RPP - 1) / RPP;
  static constexpr int WROWS = KS * KS * BN;
  static constexpr int NW = (WROWS + RPP - 1) / RPP;
  static constexpr int WN = 4 / WM;
  static constexpr int MB = 4 / WM;
  static constexpr int NB = BN / 32 / WN;
  static constexpr int LDS_FLOATS = NPIX * S + WROWS * S;
  static_assert(256 % Q == 0, "Q must divide 256");
  static_assert(BN % (32 * WN) == 0, "BN/WN must be a multiple of 32");
  static_assert(KC % 8 == 0, "KC multiple of 8");
};

template <int KS, int STRIDE, bool UP, int KC, int BN, int WM>
__global__ void __launch_bounds__(256, 2) conv_mfma_f32_kernel(const ConvParams p) {
  using Cfg = ConvCfg<KS, STRIDE, UP, KC, BN, WM>;
  constexpr int TH = Cfg::TH, TW = Cfg::TW, PAD = Cfg::PAD, HWD = Cfg::HWD, NPIX = Cfg::NPIX;
  constexpr int S = Cfg::S, Q = Cfg::Q, RPP = Cfg::RPP, NIN = Cfg::NIN, WROWS = Cfg::WROWS, NW = Cfg::NW;
  constexpr int WN = Cfg::WN, MB = Cfg::MB, NB = Cfg::NB;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sIn = smem;
  float* sW = smem + NPIX * S;
  const int Cin = p.C0 + p.C1;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  // ---- workgroup -> (image, pixel tile, Cout tile); XCD-aware: the Cout tiles of
  // one pixel tile and neighbouring pixel tiles are dealt to the same XCD (L2) ----
  const int nco = p.Cout_pad / BN;
  const int tilesX = (p.Wout + TW - 1) / TW, tilesY = (p.Hout + TH - 1) / TH;
  const int bid = xcd_block_id(blockIdx.x, gridDim.x);
  const int cot = bid % nco;
  int pt = bid / nco;
  const int tx = pt % tilesX;
  pt /= tilesX;
  const int ty = pt % tilesY;
  const int n = pt / tilesY;
  const int oy0 = ty * TH, ox0 = tx * TW, co0 = cot * BN;

  const bool gn = p.gn_scale != nullptr;

  // ---- chunk-invariant staging indices ----
  const int q = tid % Q;      // float4 slot inside the KC chunk
  const int row0 = tid / Q;   // first LDS row this thread fills
  int in_pix[NIN];            // source pixel index, -1 = zero padding, -2 = no row
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    const int pix = row0 + i * RPP;
    int v = -2;
    if (pix < NPIX) {
      const int hy = pix / HWD, hx = pix % HWD;
      const int iy = oy0 * STRIDE - PAD + hy, ix = ox0 * STRIDE - PAD + hx;
      if (UP) {
        const bool ok = iy >= 0 && iy < p.Hout && ix >= 0 && ix < p.Wout;
        v = ok ? (n * p.Hin + (iy >> 1)) * p.Win + (ix >> 1) : -1;   // nearest x2: src = floor(dst/2)
      } else {
        const bool ok = iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
        v = ok ? (n * p.Hin + iy) * p.Win + ix : -1;
      }
    }
    in_pix[i] = v;
  }

  f32x4 rin[NIN];
  f32x4 rw[NW];
  unsigned rmask[NIN];                 // train-mode dropout: 4 keep bytes per staged quad (all ones when off)
#pragma unroll
  for (int i = 0; i < NIN; ++i) rmask[i] = 0x01010101u;
  f32x4 rsc = {1.f, 1.f, 1.f, 1.f}, rsh = {0.f, 0.f, 0.f, 0.f};
  auto prefetch = [&](int kc) {
    const int cbase = kc * KC;
    const float* base;
    int Cs, cc;
    if (cbase < p.C0) { base = p.x0; Cs = p.C0; cc = cbase + q * 4; }
    else { base = p.x1; Cs = p.C1; cc = cbase - p.C0 + q * 4; }
    if (gn) {   // y = x*scale + shift, per (image, channel): travels with the input prefetch
      rsc = *reinterpret_cast<const f32x4*>(p.gn_scale + (size_t)n * Cin + cbase + q * 4);
      rsh = *reinterpret_cast<const f32x4*>(p.gn_shift + (size_t)n * Cin + cbase + q * 4);
    }
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (in_pix[i] >= 0) v = *reinterpret_cast<const f32x4*>(base + (size_t)in_pix[i] * Cs + cc);
      rin[i] = v;
      if (p.drop_mask && in_pix[i] >= 0) rmask[i] = *reinterpret_cast<const unsigned*>(p.drop_mask + (size_t)in_pix[i] * Cs + cc);
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int row = row0 + i * RPP;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < WROWS) {
        const int tap = row / BN, co = row % BN;
        v = *reinterpret_cast<const f32x4*>(p.w + ((size_t)tap * p.Cout_pad + co0 + co) * p.Cin_pad + cbase + q * 4);
      }
      rw[i] = v;
    }
  };
  auto stage = [&](int kc) {
    const f32x4 sc = rsc, sh = rsh;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      if (in_pix[i] == -2) continue;
      f32x4 v = rin[i];
      if (gn && in_pix[i] >= 0) {   // conv zero-pads the ACTIVATED tensor
        v = gn_act4(v, sc, sh, p.gn_plain);
        if (p.drop_mask) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = ((rmask[i] >> (8 * e)) & 0xffu) ? v[e] * p.drop_scale : 0.f;
        }
      }
      *reinterpret_cast<f32x4*>(sIn + (row0 + i * RPP) * S + q * 4) = v;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int row = row0 + i * RPP;
      if (row < WROWS) *reinterpret_cast<f32x4*>(sW + row * S + q * 4) = rw[i];
    }
  };

  // ---- MFMA operand addresses (floats).  A: lane l -> pixel row l&31, k-quad l>>5 ----
  const int r31 = lane & 31, h = lane >> 5;
  int abase[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int pp = (wm * MB + mb) * 32 + r31;
    const int pr = pp / TW, pc = pp % TW;
    abase[mb] = ((pr * STRIDE) * HWD + pc * STRIDE) * S + 4 * h;
  }
  int bbase[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) bbase[nb] = ((wn * NB + nb) * 32 + r31) * S + 4 * h;

  f32x16 acc[MB][NB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.f;

  const int nk = p.Cin_pad / KC;
  prefetch(0);
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();   // previous chunk's LDS reads done (and scale/shift visible)
    stage(kc);
    __syncthreads();
    if (kc + 1 < nk) prefetch(kc + 1);   // in flight under the MFMAs below
#pragma unroll
    for (int tap = 0; tap < KS * KS; ++tap) {
      const int ky = tap / KS, kx = tap % KS;
      const int aoff = (ky * HWD + kx) * S;
      const int boff = tap * BN * S;
#pragma unroll
      for (int ks = 0; ks < KC / 8; ++ks) {
        f32x4 a[MB], b[NB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) a[mb] = *reinterpret_cast<const f32x4*>(sIn + abase[mb] + aoff + ks * 8);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) b[nb] = *reinterpret_cast<const f32x4*>(sW + bbase[nb] + boff + ks * 8);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
              acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb][s], b[nb][s], acc[mb][nb], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: C/D map col = lane&31 (Cout), row = (i&3) + 8*(i>>2) + 4*(lane>>5) (pixel).
  // `res` may alias `out` (in-place residual), so ALL residual loads are issued before the
  // first store.  Interior tiles take a branch-free path (per-element bounds branches force a
  // vmcnt(0) before every store).  Each lane also sums its outputs (sum, sumsq) per channel:
  // the GroupNorm statistics of the consumer, reduced over the workgroup in a fixed order. ----
  float s1[NB], s2[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) s1[nb] = s2[nb] = 0.f;
  // out_bf16 (bf16 mode, the 6-channel input conv only): bf16 stores through the bounds-checked path
  if ((oy0 + TH <= p.Hout) && (ox0 + TW <= p.Wout) && (co0 + BN <= p.Cout) && !p.out_bf16) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int co = co0 + (wn * NB + nb) * 32 + r31;
      float add = p.bias[co];
      if (p.temb) add += p.temb[(size_t)n * p.temb_stride + p.temb_off + co];
      size_t offs[MB][16];
      float rv[MB][16];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int pp = (wm * MB + mb) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          offs[mb][i] = ((size_t)(n * p.Hout + oy0 + pp / TW) * p.Wout + ox0 + pp % TW) * p.Cout + co;
          rv[mb][i] = p.res ? p.res[offs[mb][i]] : 0.f;
        }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc[mb][nb][i] + add + rv[mb][i];
          p.out[offs[mb][i]] = v;
          s1[nb] += v;
          s2[nb] += v * v;
        }
    }
  } else {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int co = co0 + (wn * NB + nb) * 32 + r31;
      const bool cok = co < p.Cout;
      float add = 0.f;
      if (cok) {
        add = p.bias[co];
        if (p.temb) add += p.temb[(size_t)n * p.temb_stride + p.temb_off + co];
      }
      float rv[MB][16];
      if (p.res) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int pp = (wm * MB + mb) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const int oy = oy0 + pp / TW, ox = ox0 + pp % TW;
            const bool ok = cok && oy < p.Hout && ox < p.Wout;
            const size_t off = ((size_t)(n * p.Hout + oy) * p.Wout + ox) * p.Cout + co;
            rv[mb][i] = ok ? p.res[off] : 0.f;
          }
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int pp = (wm * MB + mb) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          const int oy = oy0 + pp / TW, ox = ox0 + pp % TW;
          if (cok && oy < p.Hout && ox < p.Wout) {
            const size_t off = ((size_t)(n * p.Hout + oy) * p.Wout + ox) * p.Cout + co;
            float v = acc[mb][nb][i] + add;
            if (p.res) v += rv[mb][i];
            if (p.out_bf16) reinterpret_cast<unsigned short*>(p.out)[off] = f32_to_16_bits(v, p.out_bf16);   // 1 bf16, 2 f16
            else p.out[off] = v;
            s1[nb] += v;
            s2[nb] += v * v;
          }
        }
      }
    }
  }
  if (p.part_out) {
    __syncthreads();                     // every wave is done with the LDS tiles
    float* sp = smem;                    // [WM][BN][2]
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float a = s1[nb] + __shfl_xor(s1[nb], 32, 64), b = s2[nb] + __shfl_xor(s2[nb], 32, 64);
      if (h == 0) {
        const int cl = (wn * NB + nb) * 32 + r31;
        sp[(wm * BN + cl) * 2 + 0] = a;
        sp[(wm * BN + cl) * 2 + 1] = b;
      }
    }
    __syncthreads();
    if (tid < BN && co0 + tid < p.Cout) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w = 0; w < WM; ++w) { a += sp[(w * BN + tid) * 2 + 0]; b += sp[(w * BN + tid) * 2 + 1]; }
      float* dst = p.part_out + (((size_t)n * (tilesX * tilesY) + ty * tilesX + tx) * p.Cout + co0 + tid) * 2;
      dst[0] = a;
      dst[1] = b;
    }
  }
}

template <int KS, int STRIDE, bool UP, int KC, int BN, int WM>
static hipError_t launch_conv_t(const ConvParams& p, hipStream_t s, int* tiles) {
  using Cfg = ConvCfg<KS, STRIDE, UP, KC, BN, WM>;
  auto kfn = conv_mfma_f32_kernel<KS, STRIDE, UP, KC, BN, WM>;
  const size_t lds = (size_t)Cfg::LDS_FLOATS * sizeof(float);
  const int tilesX = (p.Wout + Cfg::TW - 1) / Cfg::TW, tilesY = (p.Hout + Cfg::TH - 1) / Cfg::TH;
  const int nwg = p.N * tilesX * tilesY * (p.Cout_pad / BN);
  if (tiles) *tiles = tilesX * tilesY;
  hipLaunchKernelGGL(kfn, dim3(nwg), dim3(256), lds, s, p);
  return hipGetLastError();
}

template <int KS, int STRIDE, bool UP, int KC, int BN, int WM>
static hipError_t init_conv_t() {
  auto kfn = conv_mfma_f32_kernel<KS, STRIDE, UP, KC, BN, WM>;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// every instantiation the dispatcher below can pick: X(KS, STRIDE, UP, KC, BN, WM)
#define FDSR_CONV_INSTANCES(X)                                                          \
  X(3, 1, false, 8, 32, 4) X(3, 1, false, 8, 64, 2) X(3, 1, false, 16, 32, 4) X(3, 1, false, 16, 64, 2) \
  X(3, 2, false, 16, 32, 4) X(3, 2, false, 16, 64, 2) X(3, 1, true, 16, 32, 4) X(3, 1, true, 16, 64, 2)   \
  X(1, 1, false, 64, 32, 4) X(1, 1, false, 64, 64, 2) X(1, 1, false, 32, 32, 4) X(1, 1, false, 32, 64, 2) \
  X(1, 1, false, 16, 32, 4) X(1, 1, false, 16, 64, 2)

void conv_tile_config(ConvKind kind, int C0, int C1, int Cout, int* KC, int* BN) {
  *BN = Cout <= 32 ? 32 : 64;
  if (kind == CONV1) {
    if (C0 % 64 == 0 && C1 % 64 == 0) *KC = 64;
    else if (C0 % 32 == 0 && C1 % 32 == 0) *KC = 32;
    else *KC = 16;
  } else {
    *KC = (C0 + C1 <= 8) ? 8 : 16;
  }
}

hipError_t launch_conv(ConvKind kind, const ConvParams& p, hipStream_t s, int* tiles) {
  int KC, BN;
  conv_tile_config(kind, p.C0, p.C1, p.Cout, &KC, &BN);
  int ks = kind == CONV1 ? 1 : 3, stride = kind == CONV3_S2 ? 2 : 1;
  bool up = kind == CONV3_UP;
#define X(KS_, ST_, UP_, KC_, BN_, WM_) \
  if (ks == KS_ && stride == ST_ && up == UP_ && KC == KC_ && BN == BN_) return launch_conv_t<KS_, ST_, UP_, KC_, BN_, WM_>(p, s, tiles);
  FDSR_CONV_INSTANCES(X)
#undef X
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// GroupNorm finalisation from the producers' per-tile partial sums
// ---------------------------------------------------------------------------
// grid = (N, G): one workgroup finalises one group of one image.  Thread (ch, slice): channel ch of
// the group's cpg channels, tiles t = slice, slice + S, ... in order; the 256 slot sums are then
// folded by one wave in a fixed order (bitwise reproducible, no atomics).
__global__ void __launch_bounds__(256) gn_finalize_kernel(const GnFinalizeParams p) {
  __shared__ double sd[256][2];
  __shared__ double gs[2];
  const int C = p.C0 + p.C1, tid = threadIdx.x, n = blockIdx.x, g = blockIdx.y;
  const int cpg = C / p.G;                  // <= 64 (launcher checks)
  const int S = 256 / cpg;                  // tile slices per channel
  const int ch = tid % cpg, slice = tid / cpg;
  const int c = g * cpg + ch;
  // the affine parameters of this thread's channel are fetched NOW, beside the partials: issued after the fold they were one more
  // exposed memory round trip in a kernel that is nothing but latency (45 of these launches per forward)
  float gam = 0.f, bet = 0.f, f_s = 0.f, f_t = 0.f;
  if (tid < cpg) {
    const int cc = g * cpg + tid;
    gam = p.gamma[cc];
    bet = p.beta[cc];
    if (p.film) {
      const float* f = p.film + (size_t)n * p.film_stride + p.film_off;
      f_s = f[cc];
      f_t = f[C + cc];
    }
  }
  double a = 0.0, b = 0.0;
  if (slice < S) {
    const float* part;
    int nt, Cs, cc;
    if (c < p.C0) { part = p.part0; nt = p.nt0; Cs = p.C0; cc = c; } else { part = p.part1; nt = p.nt1; Cs = p.C1; cc = c - p.C0; }
    const float* src = part + ((size_t)n * nt * Cs + cc) * 2;
    // eight tiles per trip, all eight loads in flight before the first add (tiles past the end re-read the last one and add 0: the same
    // sums in the same order); a trip is one memory round trip, and up to 8 S tiles -- every B = 1 shape -- need one trip only
    for (int t0 = slice; t0 < nt; t0 += 8 * S) {
      float2 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float2*>(src + (size_t)min(t0 + j * S, nt - 1) * Cs * 2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = t0 + j * S < nt;
        a += in ? (double)v[j].x : 0.0;
        b += in ? (double)v[j].y : 0.0;
      }
    }
  }
  sd[tid][0] = a;
  sd[tid][1] = b;
  __syncthreads();
  if (tid < 64) {   // one wave folds the 256 slots: four strided adds, then a butterfly (same order every run)
    double ga = 0.0, gb = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { ga += sd[tid + 64 * k][0]; gb += sd[tid + 64 * k][1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ga += __shfl_xor(ga, o, 64); gb += __shfl_xor(gb, o, 64); }
    if (tid == 0) {
      const double inv = 1.0 / ((double)cpg * (double)p.HW);
      const double mean = ga * inv;
      double var = gb * inv - mean * mean;
      var = var < 0.0 ? 0.0 : var;
      gs[0] = mean;
      gs[1] = 1.0 / sqrt(var + (double)p.eps);
      if (p.stats) {
        p.stats[((size_t)n * p.G + g) * 2] = (float)gs[0];
        p.stats[((size_t)n * p.G + g) * 2 + 1] = (float)gs[1];
      }
    }
  }
  __syncthreads();
  if (tid < cpg) {
    const int cc = g * cpg + tid;
    float sc = (float)gs[1] * gam;
    float sh = bet - (float)gs[0] * sc;
    if (p.film) {   // (x_hat*gamma + beta) * (1 + s) + t
      const float one_s = 1.0f + f_s;
      sc *= one_s;
      sh = sh * one_s + f_t;
    }
    p.scale[(size_t)n * C + cc] = sc;
    p.shift[(size_t)n * C + cc] = sh;
  }
}

hipError_t launch_gn_finalize(const GnFinalizeParams& p, hipStream_t s) {
  const int C = p.C0 + p.C1;
  if (C % p.G || C / p.G > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(p.N, p.G), dim3(256), 0, s, p);
  return hipGetLastError();
}

Tunables g_tun;

int set_tunable(const char* name, long long v) {
  const std::string n(name ? name : "");
  if (n == "rider") g_tun.rider = (int)v;
  else if (n == "up2") g_tun.up2 = (int)v;
  else if (n == "th_min_wgs") g_tun.th_min_wgs = (long)v;
  else if (n == "splitk") g_tun.splitk = (int)v;
  else if (n == "sk_target") g_tun.sk_target = (int)v;
  else if (n == "wgrad_form") g_tun.wgrad_form = (int)v;
  else if (n == "wgrad_colsum") g_tun.wgrad_colsum = (int)v;
  else if (n == "wgrad_f32") g_tun.wgrad_f32 = (int)v;
  else if (n == "gnb_fuse") g_tun.gnb_fuse = (int)v;
  else if (n == "drop_stage") g_tun.drop_stage = (int)v;
  else if (n == "wgrad_big_bytes") g_tun.wgrad_big_bytes = v;
  else if (n == "k32") g_tun.k32 = (int)v;
  else if (n == "k32_sb_min_wgs") g_tun.k32_sb_min_wgs = (long)v;
  else if (n == "k32_stagger") g_tun.k32_stagger = (int)v;
  else if (n == "strip") g_tun.strip = (int)v;
  else if (n == "strip_min_wgs") g_tun.strip_min_wgs = (long)v;
  else if (n == "gn_consumer") g_tun.gn_consumer = (int)v;
  else if (n == "bf16_f16x3_steps") g_tun.bf16_f16x3_steps = (int)v;
  else if (n == "sat_guard") g_tun.sat_guard = (int)v;
  else if (n == "tail") g_tun.tail = (int)v;
  else if (n == "knockout") g_tun.knockout = (int)v;
  else if (n == "drop_image_offset") g_tun.drop_image_offset = (int)v;
  else return -1;
  ++g_tun.epoch;
  return 0;
}

int conv_max_tiles(int H, int W) {
  // f32 kernel: 8x16 tiles; 16-bit kernels: TH x 32 with TH >= 2
  const int a = ((H + 7) / 8) * ((W + 15) / 16), b = ((H + 1) / 2) * ((W + 31) / 32);
  return a > b ? a : b;
}

// ---------------------------------------------------------------------------
// noise-level embedding + all per-block shifts
// ---------------------------------------------------------------------------
#define FDSR_TEMB_ROWS 512
__global__ void __launch_bounds__(256) temb_kernel(const TembParams p) {
  extern __shared__ __attribute__((aligned(16))) float st[];   // enc[E] | hid[Hd] | t[Td]
  const int E = p.enc_dim ? p.enc_dim : p.inner, hid = p.hid_dim ? p.hid_dim : 4 * p.inner, Td = p.t_dim ? p.t_dim : p.inner;
  const int tid = threadIdx.x, n = blockIdx.x;
  float* enc = st;
  float* hbuf = st + E;
  float* tv = hbuf + hid;
  const float nl = p.nl_dev ? p.nl_dev[n] : p.nl_scalar;   // noise level, or the integer time (SR3 / GDP variants)
  const int half = E / 2;
  for (int k = tid; k < half; k += 256) {   // unet.py:27-35 / ddpm_modules TimeEmbedding: cat([sin, cos], -1); GDP: cat([cos, sin])
    const float e = nl * p.freq[k];
    enc[p.cos_first ? half + k : k] = sinf(e);
    enc[p.cos_first ? k : half + k] = cosf(e);
  }
  __syncthreads();
  for (int j = tid; j < hid; j += 256) {
    float a = p.b1[j];
    const float* w = p.w1 + (size_t)j * E;
    for (int k = 0; k < E; ++k) a = fmaf(w[k], enc[k], a);
    hbuf[j] = a / (1.0f + expf(-a));
  }
  __syncthreads();
  for (int j = tid; j < Td; j += 256) {
    float a = p.b2[j];
    const float* w = p.w2 + (size_t)j * hid;
    for (int k = 0; k < hid; ++k) a = fmaf(w[k], hbuf[k], a);
    // SR3 (ddpm_modules/unet.py:81-84) and GDP (gdp_modules/unet.py:336-342): the per-block Linear is applied to Swish(t)
    tv[j] = p.swish_block ? a / (1.0f + expf(-a)) : a;
  }
  __syncthreads();
  // grid.y: blocks of FDSR_TEMB_ROWS rows of the per-block Linears (every workgroup repeats the small MLP above: the GDP sibling at
  // the reference's width has 30 000 rows of 512 columns, 15 M multiply-adds per image -- 2.4 ms in ONE workgroup)
  const int o_end = min(p.TE, (int)(blockIdx.y + 1) * FDSR_TEMB_ROWS);
  for (int o = blockIdx.y * FDSR_TEMB_ROWS + tid; o < o_end; o += 256) {
    float a = p.bn[o];
    const float* w = p.wn + (size_t)o * Td;
    for (int k = 0; k < Td; ++k) a = fmaf(w[k], tv[k], a);
    p.temb[(size_t)n * p.TE + o] = a;
  }
}

hipError_t launch_temb(const TembParams& p, hipStream_t s) {
  const int E = p.enc_dim ? p.enc_dim : p.inner, hid = p.hid_dim ? p.hid_dim : 4 * p.inner, Td = p.t_dim ? p.t_dim : p.inner;
  hipLaunchKernelGGL(temb_kernel, dim3(p.N, (p.TE + FDSR_TEMB_ROWS - 1) / FDSR_TEMB_ROWS), dim3(256), (size_t)(E + hid + Td) * sizeof(float), s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// CLAM gate: global avg / max pool -> shared MLP -> sigmoid       (unet.py:123-149)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// four consecutive channels of an activation tensor kept as fp32 (BF = 0), bf16 (BF = 1, bf16 mode) or f16 (BF = 2, f16 mode)
template <int BF>
__device__ __forceinline__ f32x4 ldq(const float* base, size_t idx) {
  if (BF == 2) return ActIO<PREC_F16>::widen(ActIO<PREC_F16>::load4(base, idx));
  if (BF) {
    const uint2 q = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(base) + idx);
    f32x4 r = {__builtin_bit_cast(float, q.x << 16), __builtin_bit_cast(float, q.x & 0xffff0000u),
               __builtin_bit_cast(float, q.y << 16), __builtin_bit_cast(float, q.y & 0xffff0000u)};
    return r;
  }
  return *reinterpret_cast<const f32x4*>(base + idx);
}
template <int BF>
__device__ __forceinline__ void stq(float* base, size_t idx, f32x4 v) {
  if (BF == 2) {
    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(base) + idx) = pack4_16<PREC_F16>(v);
  } else if (BF) {
    uint2 pk;
    pk.x = (unsigned)__builtin_bit_cast(unsigned short, (__bf16)v[0]) | ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)v[1]) << 16);
    pk.y = (unsigned)__builtin_bit_cast(unsigned short, (__bf16)v[2]) | ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)v[3]) << 16);
    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(base) + idx) = pk;
  } else {
    *reinterpret_cast<f32x4*>(base + idx) = v;
  }
}

// Phase 1, grid (FDSR_CLAM_SLICES, N): per-channel sum and maximum of one pixel slice.
template <int BF>
__global__ void __launch_bounds__(256) clam_pool_kernel(const float* __restrict__ x, int HW, int C, float* __restrict__ pool) {
  __shared__ __attribute__((aligned(16))) float ps[256 * 8];
  const int tid = threadIdx.x, sl = blockIdx.x, n = blockIdx.y;
  const int cq = C >> 2, rows = 256 / cq, c4 = tid % cq, r = tid / cq;
  const int p0 = (int)((long)sl * HW / FDSR_CLAM_SLICES), p1 = (int)((long)(sl + 1) * HW / FDSR_CLAM_SLICES);
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (r < rows) {
    const size_t base = (size_t)n * HW * C + c4 * 4;
    for (int pix = p0 + r; pix < p1; pix += rows) {
      const f32x4 v = ldq<BF>(x, base + (size_t)pix * C);
      s += v;
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
    }
    *reinterpret_cast<f32x4*>(ps + (r * cq + c4) * 8) = s;
    *reinterpret_cast<f32x4*>(ps + (r * cq + c4) * 8 + 4) = m;
  }
  __syncthreads();
  if (tid < cq) {
    f32x4 a = *reinterpret_cast<const f32x4*>(ps + tid * 8), b = *reinterpret_cast<const f32x4*>(ps + tid * 8 + 4);
    for (int rr = 1; rr < rows; ++rr) {
      a += *reinterpret_cast<const f32x4*>(ps + (rr * cq + tid) * 8);
      const f32x4 q = *reinterpret_cast<const f32x4*>(ps + (rr * cq + tid) * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = fmaxf(b[e], q[e]);
    }
    float* dst = pool + (((size_t)n * FDSR_CLAM_SLICES + sl) * C + tid * 4) * 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { dst[2 * e] = a[e]; dst[2 * e + 1] = b[e]; }
  }
}

// Phase 2, grid (N): fold the slices in order, then the shared MLP on both pooled vectors.
__global__ void __launch_bounds__(256) clam_gate_kernel(const float* __restrict__ pool, int HW, int C, const float* __restrict__ fc1,
                                                        const float* __restrict__ fc2, int Cr, float* gate) {
  extern __shared__ __attribute__((aligned(16))) float sm[];   // avg[C] | mx[C] | ha[Cr] | hm[Cr]
  const int tid = threadIdx.x, n = blockIdx.x;
  float* avg = sm;
  float* mx = avg + C;
  float* ha = mx + C;
  float* hm = ha + Cr;
  for (int cc = tid; cc < C; cc += 256) {
    float s = 0.f, m = -INFINITY;
    const float* src = pool + ((size_t)n * FDSR_CLAM_SLICES * C + cc) * 2;
#pragma unroll 8
    for (int sl = 0; sl < FDSR_CLAM_SLICES; ++sl) {
      const float2 v = *reinterpret_cast<const float2*>(src + (size_t)sl * C * 2);
      s += v.x;
      m = fmaxf(m, v.y);
    }
    avg[cc] = s / (float)HW;
    mx[cc] = m;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < 2 * Cr; j += 4) {   // fc1 + ReLU on both pooled vectors
    const int jj = j % Cr;
    const float* v = j < Cr ? avg : mx;
    float a = 0.f;
    for (int k = lane; k < C; k += 64) a = fmaf(fc1[(size_t)jj * C + k], v[k], a);
    a = wave_sum(a);
    if (lane == 0) (j < Cr ? ha : hm)[jj] = fmaxf(a, 0.f);
  }
  __syncthreads();
  for (int cc = tid; cc < C; cc += 256) {
    float a = 0.f, b = 0.f;
    for (int j = 0; j < Cr; ++j) { a = fmaf(fc2[(size_t)cc * Cr + j], ha[j], a); b = fmaf(fc2[(size_t)cc * Cr + j], hm[j], b); }
    const float o = a + b;
    gate[(size_t)n * C + cc] = 1.0f / (1.0f + expf(-o));
  }
}

size_t clam_slam_scratch_floats(int N, int HW, int C) {
  return (size_t)N * C + (size_t)N * FDSR_CLAM_SLICES * C * 2 + (size_t)N * 2 * HW;
}

hipError_t launch_clam_gate(const float* x, int N, int HW, int C, const float* fc1, const float* fc2, int Cr,
                            float* scratch, hipStream_t s, int act_bf16) {
  if (C > 1024 || (C & 3)) return hipErrorInvalidValue;
  float* gate = scratch;
  float* pool = scratch + (size_t)N * C;
  if (act_bf16 == 2) hipLaunchKernelGGL(clam_pool_kernel<2>, dim3(FDSR_CLAM_SLICES, N), dim3(256), 0, s, x, HW, C, pool);
  else if (act_bf16) hipLaunchKernelGGL(clam_pool_kernel<1>, dim3(FDSR_CLAM_SLICES, N), dim3(256), 0, s, x, HW, C, pool);
  else hipLaunchKernelGGL(clam_pool_kernel<0>, dim3(FDSR_CLAM_SLICES, N), dim3(256), 0, s, x, HW, C, pool);
  const size_t lds = (size_t)(2 * C + 2 * Cr) * sizeof(float);
  hipLaunchKernelGGL(clam_gate_kernel, dim3(N), dim3(256), lds, s, pool, HW, C, fc1, fc2, Cr, gate);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// SLAM on y = x*gate: channel mean/max -> 7x7 conv -> sigmoid -> scale   (unet.py:151-173)
// ---------------------------------------------------------------------------
// Phase 1, grid (ceil(HW/16), N): one wave per pixel, map[n][0] = mean_c y, map[n][1] = max_c y.
template <int BF>
__global__ void __launch_bounds__(256) slam_map_kernel(const float* __restrict__ x, const float* __restrict__ gate, int HW, int C,
                                                       float* __restrict__ map) {
  const int tid = threadIdx.x, n = blockIdx.y, wave = tid >> 6, lane = tid & 63;
  const size_t xb = (size_t)n * HW * C;
  const float* gb = gate + (size_t)n * C;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pix = blockIdx.x * 16 + wave * 4 + i;
    if (pix >= HW) break;
    float s = 0.f, m = -INFINITY;
    for (int c = lane * 4; c < C; c += 256) {
      const f32x4 v = ldq<BF>(x, xb + (size_t)pix * C + c);
      const f32x4 g = *reinterpret_cast<const f32x4*>(gb + c);
      const f32x4 y = g * v;
      s += (y.x + y.y) + (y.z + y.w);
      m = fmaxf(m, fmaxf(fmaxf(y.x, y.y), fmaxf(y.z, y.w)));
    }
    s = wave_sum(s);
    m = wave_max(m);
    if (lane == 0) { map[(size_t)n * 2 * HW + pix] = s / (float)C; map[(size_t)n * 2 * HW + HW + pix] = m; }
  }
}

// Phase 2, grid (tiles of 2 x 32 pixels, N): 7x7 conv + sigmoid on the map, out = sig * (gate * x), and the
// per-tile channel statistics of out (GroupNorm input of the next block, mid.1.block1).
template <int BF>
__global__ void __launch_bounds__(256) slam_apply_kernel(const float* __restrict__ x, const float* __restrict__ gate,
                                                         const float* __restrict__ map, const float* __restrict__ w7, int H, int W,
                                                         int C, float* out, float* part_out) {
  __shared__ __attribute__((aligned(16))) float red[256 * 8];
  __shared__ float sig[64];
  __shared__ float wk[98];
  __shared__ float mh[2][8][38];   // the map's halo image of this tile (2 + 6 rows x 32 + 6 columns, zero outside the map)
  const int HW = H * W, tid = threadIdx.x, tile = blockIdx.x, n = blockIdx.y;
  const int tilesX = (W + 31) / 32, tx = tile % tilesX, ty = tile / tilesX;
  // weights and halo in ONE round trip: every load unconditional on a clamped address (the 98 map reads per pixel used to sit behind
  // `continue`s, each waiting for its own round trip: 15 of this kernel's 19 us at B = 1)
  {
    const float wv = w7[min(tid, 97)];
    const float* mp = map + (size_t)n * 2 * HW;
    float hv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = min(tid + 256 * i, 2 * 8 * 38 - 1);
      const int ch = e / (8 * 38), r = (e / 38) % 8, c = e % 38;
      const int iy = ty * 2 + r - 3, ix = tx * 32 + c - 3;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float v = mp[ch * HW + min(max(iy, 0), H - 1) * W + min(max(ix, 0), W - 1)];
      hv[i] = in ? v : 0.f;
    }
    if (tid < 98) wk[tid] = wv;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = tid + 256 * i;
      if (e < 2 * 8 * 38) (&mh[0][0][0])[e] = hv[i];
    }
  }
  __syncthreads();
  if (tid < 64) {
    const int ry = tid >> 5, rx = tid & 31;
    float a = 0.f;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
      for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) a = fmaf(wk[(ch * 7 + ky) * 7 + kx], mh[ch][ry + ky][rx + kx], a);   // (zero taps outside the map: the same sum)
    sig[tid] = 1.0f / (1.0f + expf(-a));
  }
  __syncthreads();
  const int cq = C >> 2, groups = 256 / cq, c4 = tid % cq, g = tid / cq;
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  {
    // eight pixels per trip, their loads in flight together (clamped addresses; the store and the sums take the value only where the
    // pixel exists) -- one round trip per trip instead of one per pixel
    const f32x4 gv = *reinterpret_cast<const f32x4*>(gate + (size_t)n * C + c4 * 4);
    for (int px0 = g; px0 < 64; px0 += 8 * groups) {
      f32x4 v[8];
      size_t o[8];
      bool ok[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int px = px0 + j * groups, pc = min(px, 63);
        const int y = ty * 2 + (pc >> 5), xx = tx * 32 + (pc & 31);
        ok[j] = g < groups && px < 64 && y < H && xx < W;
        o[j] = ((size_t)n * HW + (size_t)min(y, H - 1) * W + min(xx, W - 1)) * C + c4 * 4;
        v[j] = ldq<BF>(x, o[j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 r = sig[min(px0 + j * groups, 63)] * (gv * v[j]);
        if (ok[j]) stq<BF>(out, o[j], r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float q = ok[j] ? r[e] : 0.f;
          s1[e] += q;
          s2[e] += q * q;
        }
      }
    }
  }
  if (part_out) {
    if (g < groups) {
      *reinterpret_cast<f32x4*>(red + (g * cq + c4) * 8) = s1;
      *reinterpret_cast<f32x4*>(red + (g * cq + c4) * 8 + 4) = s2;
    }
    __syncthreads();
    if (tid < cq) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
      for (int gg = 0; gg < groups; ++gg) {
        a += *reinterpret_cast<const f32x4*>(red + (gg * cq + tid) * 8);
        b += *reinterpret_cast<const f32x4*>(red + (gg * cq + tid) * 8 + 4);
      }
      float* dst = part_out + (((size_t)n * gridDim.x + tile) * C + tid * 4) * 2;
#pragma unroll
      for (int e = 0; e < 4; ++e) { dst[2 * e] = a[e]; dst[2 * e + 1] = b[e]; }
    }
  }
}

hipError_t launch_slam(const float* x, float* scratch, const float* w7, int N, int H, int W, int C, float* out,
                       float* part_out, hipStream_t s, int* tiles, int act_bf16) {
  if (C > 1024 || (C & 3)) return hipErrorInvalidValue;
  const int HW = H * W;
  const float* gate = scratch;
  float* map = scratch + (size_t)N * C + (size_t)N * FDSR_CLAM_SLICES * C * 2;
  if (act_bf16 == 2) hipLaunchKernelGGL(slam_map_kernel<2>, dim3((HW + 15) / 16, N), dim3(256), 0, s, x, gate, HW, C, map);
  else if (act_bf16) hipLaunchKernelGGL(slam_map_kernel<1>, dim3((HW + 15) / 16, N), dim3(256), 0, s, x, gate, HW, C, map);
  else hipLaunchKernelGGL(slam_map_kernel<0>, dim3((HW + 15) / 16, N), dim3(256), 0, s, x, gate, HW, C, map);
  const int nt = ((W + 31) / 32) * ((H + 1) / 2);
  if (tiles) *tiles = nt;
  if (act_bf16 == 2) hipLaunchKernelGGL(slam_apply_kernel<2>, dim3(nt, N), dim3(256), 0, s, x, gate, map, w7, H, W, C, out, part_out);
  else if (act_bf16) hipLaunchKernelGGL(slam_apply_kernel<1>, dim3(nt, N), dim3(256), 0, s, x, gate, map, w7, H, W, C, out, part_out);
  else hipLaunchKernelGGL(slam_apply_kernel<0>, dim3(nt, N), dim3(256), 0, s, x, gate, map, w7, H, W, C, out, part_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// boundary layout changes
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ src, float* __restrict__ dst, int Csrc,
                                                           int HW, int Cdst, int c_off, int zero_rest, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t n = i / HW, pix = i % HW;
  float* d = dst + i * Cdst;
  if (zero_rest)
    for (int c = 0; c < Cdst; ++c)
      if (c < c_off || c >= c_off + Csrc) d[c] = 0.f;
  for (int c = 0; c < Csrc; ++c) d[c_off + c] = src[(n * Csrc + c) * HW + pix];
}

hipError_t launch_nchw_to_nhwc(const float* src, float* dst, int N, int Csrc, int H, int W, int Cdst, int c_off,
                               int zero_rest, hipStream_t s) {
  const size_t total = (size_t)N * H * W;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, Csrc, H * W,
                     Cdst, c_off, zero_rest, total);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int HW,
                                                           int stride, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t n = i / HW, pix = i % HW;
  for (int c = 0; c < C; ++c) dst[(n * C + c) * HW + pix] = src[i * stride + c];
}

hipError_t launch_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, int stride, hipStream_t s) {
  const size_t total = (size_t)N * H * W;
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, C, H * W, stride,
                     total);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// engine-side N(0,1): Philox4x32-10 (Salmon et al., SC'11) + Box-Muller
// ---------------------------------------------------------------------------
__global__ void rng_advance_kernel(unsigned long long* rng) {
  if (threadIdx.x == 0 && blockIdx.x == 0) rng[1] += 1ull;
}
hipError_t launch_rng_advance(unsigned long long* rng, hipStream_t s) {
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(64), 0, s, rng);
  return hipGetLastError();
}

// four keep bytes per Philox call: byte e of quad i = (word e >= p * 2^32)
__global__ void __launch_bounds__(256) dropout_mask_kernel(unsigned* __restrict__ mask4, size_t nquads, unsigned long long seed,
                                                           unsigned step, unsigned slot, unsigned thresh, size_t quad0) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nquads) return;
  const size_t gi = i + quad0;   // counter = position in the FULL batch (a shard of a larger batch draws its own images' masks)
  unsigned c0 = (unsigned)gi, c1 = (unsigned)(gi >> 32), c2 = slot, c3 = step;
  unsigned k0 = (unsigned)seed ^ 0x44524F50u /* 'DROP' */, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  mask4[i] = (c0 >= thresh ? 1u : 0u) | (c1 >= thresh ? 0x100u : 0u) | (c2 >= thresh ? 0x10000u : 0u) | (c3 >= thresh ? 0x1000000u : 0u);
}

hipError_t launch_dropout_mask(unsigned char* mask, size_t n, unsigned long long seed, unsigned step, unsigned slot, float p,
                               hipStream_t s, size_t first_elem) {
  if ((n & 3) || (first_elem & 3)) return hipErrorInvalidValue;
  const double t = (double)p * 4294967296.0;
  const unsigned thresh = t >= 4294967295.0 ? 0xffffffffu : (unsigned)t;
  const size_t nq = n >> 2;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, reinterpret_cast<unsigned*>(mask), nq, seed,
                     step, slot, thresh, first_elem >> 2);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) randn_plane_kernel(const unsigned long long* __restrict__ rng, float* __restrict__ dst, int HW,
                                                          int CP, int c_off, int plane, size_t total, size_t pix0, const NoiseTiles tiles) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t n = i / HW, pix = i % HW;
  float z[3];
  // counter = pixel of the FULL batch (pix0: the first pixel of a shard of a larger batch), or of the scene the images are tiles of
  randn3(rng, plane, tiles.origins ? tile_counter(tiles.origins, tiles.scene_w, tiles.W, n, pix) : i + pix0, z);
  if (CP) {   // NHWC, channels c_off..c_off+2 of the packed input
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[i * CP + c_off + c] = z[c];
  } else {    // NCHW [N,3,H,W]
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(n * 3 + c) * HW + pix] = z[c];
  }
}
hipError_t launch_randn_plane(const unsigned long long* rng, float* dst, int N, int HW, int plane, hipStream_t s, size_t first_image,
                              NoiseTiles tiles) {
  const size_t total = (size_t)N * HW;
  hipLaunchKernelGGL(randn_plane_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rng, dst, HW, 0, 0, plane, total,
                     first_image * HW, tiles);
  return hipGetLastError();
}
hipError_t launch_randn_xin(const unsigned long long* rng, float* xin, int N, int HW, int CP, hipStream_t s, int c_off, NoiseTiles tiles) {
  const size_t total = (size_t)N * HW;
  hipLaunchKernelGGL(randn_plane_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rng, xin, HW, CP, c_off, 0, total,
                     (size_t)0, tiles);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// reverse-diffusion update                                   (diffusion.py:157-190)
// ---------------------------------------------------------------------------
// one pixel of one step; both posterior kernels below run exactly this arithmetic
__device__ __forceinline__ void posterior_pixel(size_t i, int HW, int CP, const float* eps, float* xin,
                                                const float* noise, const unsigned long long* rng, int rng_plane,
                                                const NoiseTiles& tiles, float* traj, float* out, float c_recip, float c_recipm1, float coef1, float coef2, float sigma,
                                                int plain_out, int x_off, int x0_pred) {
  const size_t n = i / HW, pix = i % HW;
  float* xs = xin + i * CP;
  float z[3] = {0.f, 0.f, 0.f};
  if (rng) randn3(rng, rng_plane, tiles.origins ? tile_counter(tiles.origins, tiles.scene_w, tiles.W, n, pix) : i, z);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = xs[x_off + c];
    const float e = eps[i * 3 + c];
    // two separately rounded products, then subtract: no fma contraction
    const float a = __fmul_rn(c_recip, x);
    const float b = __fmul_rn(c_recipm1, e);
    float x0 = x0_pred ? e : __fsub_rn(a, b);                                 // GDP: the network output IS x_0
    x0 = fminf(fmaxf(x0, -1.f), 1.f);                                        // clamp_(-1, 1)  :178-179
    const float mean = __fadd_rn(__fmul_rn(coef1, x0), __fmul_rn(coef2, x));   // :161-165
    float xn = mean;
    const size_t o = (n * 3 + c) * HW + pix;
    if (noise) xn = __fadd_rn(mean, __fmul_rn(noise[o], sigma));             // :189-190
    else if (rng) xn = __fadd_rn(mean, __fmul_rn(z[c], sigma));
    xs[x_off + c] = xn;
    if (traj) traj[o] = xn;
    if (out) out[o] = plain_out ? xn : fminf(fmaxf(xn, -1.f), 1.f) / 2.0f + xs[(x_off ? 0 : 3) + c];   // res2img :275-281 (SR3: the image itself)
  }
}

__global__ void __launch_bounds__(256) posterior_kernel(const PosteriorParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)p.N * p.HW;
  if (i >= total) return;
  posterior_pixel(i, p.HW, p.CP, p.eps, p.xin, p.noise, p.rng, p.rng_plane, p.tiles, p.traj, p.out, p.c_recip, p.c_recipm1, p.coef1, p.coef2,
                  p.sigma, p.plain_out, p.x_off, p.x0_pred);
}

hipError_t launch_posterior(const PosteriorParams& p, hipStream_t s) {
  const size_t total = (size_t)p.N * p.HW;
  hipLaunchKernelGGL(posterior_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// device-resident step state (fdsr_sample_stepwise)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) step_prologue_kernel(const StepPrologueParams p) {
  __shared__ int sk;
  if (threadIdx.x == 0) sk = *p.counter;
  __syncthreads();
  // the host resets the counter before step 0 and launches exactly T steps; the clamp only keeps a misuse inside the tables
  const int k = min(max(sk, 0), p.T - 1);
  const int t = p.T - 1 - k;
  const float* row = p.temb_table + (size_t)t * p.TE;
  for (int j = threadIdx.x; j < p.TE; j += 256) p.temb_row[j] = row[j];
  if (threadIdx.x == 0) {
    StepRecord r;
    r.c_recip = p.sched[t];
    r.c_recipm1 = p.sched[p.T + t];
    r.coef1 = p.sched[2 * p.T + t];
    r.coef2 = p.sched[3 * p.T + t];
    r.sigma = p.sched[4 * p.T + t];
    r.rng_plane = k + 1;
    r.noise_plane = t > 0 ? k + 1 : -1;
    // slots hold t = T-1, T-2, ... that are multiples of traj_every: t's slot counts the multiples above it
    r.traj_slot = (t % p.traj_every == 0) ? (p.T - 1) / p.traj_every - t / p.traj_every : -1;
    r.is_last = t == 0 ? 1 : 0;
    *p.rec = r;
  }
  __syncthreads();   // every read of the counter is done before it moves
  if (threadIdx.x == 0) *p.counter = sk + 1;
}

hipError_t launch_step_prologue(const StepPrologueParams& p, hipStream_t s) {
  if (p.T < 1 || p.TE < 1 || p.traj_every < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(step_prologue_kernel, dim3(1), dim3(256), 0, s, p);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) posterior_step_kernel(const PosteriorStepParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)p.N * p.HW;
  if (i >= total) return;
  const StepRecord r = *p.rec;
  const size_t img = total * 3;
  const float* noise = (p.noise && r.noise_plane >= 0) ? p.noise + (size_t)r.noise_plane * img : nullptr;
  const unsigned long long* rng = (!p.noise && r.noise_plane >= 0) ? p.rng : nullptr;
  float* traj = (p.traj && r.traj_slot >= 0) ? p.traj + (size_t)r.traj_slot * img : nullptr;
  float* out = r.is_last ? p.out : nullptr;
  posterior_pixel(i, p.HW, p.CP, p.eps, p.xin, noise, rng, r.rng_plane, p.tiles, traj, out, r.c_recip, r.c_recipm1, r.coef1, r.coef2, r.sigma,
                  p.plain_out, p.x_off, p.x0_pred);
}

hipError_t launch_posterior_step(const PosteriorStepParams& p, hipStream_t s) {
  const size_t total = (size_t)p.N * p.HW;
  hipLaunchKernelGGL(posterior_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// tensor2img (reference core/metrics.py:16-42): clamp to [lo,hi], rescale to [0,1] in fp32,
// *255, round half to even (numpy .round()), uint8; NCHW fp32 -> HWC uint8 per image
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tensor2img_u8_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst,
                                                            int C, int HW, float lo, float hi, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t n = i / HW, pix = i % HW;
  for (int c = 0; c < C; ++c) {
    float v = src[(n * C + c) * HW + pix];
    v = fminf(fmaxf(v, lo), hi);
    v = __fdiv_rn(__fsub_rn(v, lo), __fsub_rn(hi, lo));
    dst[i * C + c] = (unsigned char)rintf(__fmul_rn(v, 255.0f));
  }
}

hipError_t launch_tensor2img_u8(const float* src, unsigned char* dst, int N, int C, int H, int W, float lo, float hi,
                                hipStream_t s) {
  const size_t total = (size_t)N * H * W;
  hipLaunchKernelGGL(tensor2img_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, C, H * W, lo, hi,
                     total);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// PIL-exact 8-bit bicubic resize (Pillow libImaging/Resample.c: fixed point, PRECISION_BITS = 22,
// horizontal pass, clip8, vertical pass, clip8) + the val-time tensor transform (uint8/255*2-1, CHW).
// bounds[X] = (first tap, tap count), kk[X][ksize] = fixed-point coefficients (host-built tables).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int clip8_fix(int v) {
  v >>= 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ void __launch_bounds__(256) resize_h_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                          const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                          int h, int w, int W, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // over N*h*W output pixels
  if (i >= total) return;
  const int X = (int)(i % W);
  const size_t row = i / W;                                  // n*h + y
  const int xmin = bounds[2 * X], cnt = bounds[2 * X + 1];
  const int* k = kk + (size_t)X * ksize;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  const unsigned char* s = src + (row * w + xmin) * 3;
  for (int x = 0; x < cnt; ++x) {
    const int c = k[x];
    a0 += s[3 * x + 0] * c;
    a1 += s[3 * x + 1] * c;
    a2 += s[3 * x + 2] * c;
  }
  unsigned char* d = dst + i * 3;
  d[0] = (unsigned char)clip8_fix(a0);
  d[1] = (unsigned char)clip8_fix(a1);
  d[2] = (unsigned char)clip8_fix(a2);
}

__global__ void __launch_bounds__(256) resize_v_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst_u8,
                                                          float* __restrict__ dst_f32, const int* __restrict__ bounds,
                                                          const int* __restrict__ kk, int ksize, int h, int H, int W,
                                                          size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // over N*H*W output pixels
  if (i >= total) return;
  const int X = (int)(i % W);
  const int Y = (int)((i / W) % H);
  const size_t n = i / ((size_t)W * H);
  const int ymin = bounds[2 * Y], cnt = bounds[2 * Y + 1];
  const int* k = kk + (size_t)Y * ksize;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  const unsigned char* s = src + ((n * h + ymin) * W + X) * 3;
  for (int y = 0; y < cnt; ++y) {
    const int c = k[y];
    a0 += s[(size_t)y * W * 3 + 0] * c;
    a1 += s[(size_t)y * W * 3 + 1] * c;
    a2 += s[(size_t)y * W * 3 + 2] * c;
  }
  const int v[3] = {clip8_fix(a0), clip8_fix(a1), clip8_fix(a2)};
  if (dst_u8) { dst_u8[i * 3 + 0] = (unsigned char)v[0]; dst_u8[i * 3 + 1] = (unsigned char)v[1]; dst_u8[i * 3 + 2] = (unsigned char)v[2]; }
  if (dst_f32) {   // ToTensor(): uint8 -> fp32 / 255; then x*2 + (-1)   (data/util.py:66-75)
    const size_t plane = (size_t)H * W, pix = (size_t)Y * W + X;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dst_f32[(n * 3 + c) * plane + pix] = __fadd_rn(__fmul_rn(__fdiv_rn((float)v[c], 255.0f), 2.0f), -1.0f);
  }
}

hipError_t launch_resize_bicubic_u8(const unsigned char* src, unsigned char* tmp, unsigned char* dst_u8, float* dst_f32, int N,
                                    int h, int w, int H, int W, const int* bounds_x, const int* kk_x, int ksize_x,
                                    const int* bounds_y, const int* kk_y, int ksize_y, hipStream_t s) {
  const size_t t1 = (size_t)N * h * W, t2 = (size_t)N * H * W;
  hipLaunchKernelGGL(resize_h_u8_kernel, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, s, src, tmp, bounds_x, kk_x, ksize_x, h, w,
                     W, t1);
  hipLaunchKernelGGL(resize_v_u8_kernel, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, s, tmp, dst_u8, dst_f32, bounds_y, kk_y,
                     ksize_y, h, H, W, t2);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// SelfAttention of the SR3 sibling (ddpm_modules/unet.py:99-127, n_head = 1) on the exact-fp32 matrix
// instruction: S = Q K^T / sqrt(C) -> row softmax -> O = P V.  q/k/v are channel slices of the
// NHWC qkv tensor [N][HW][3C]; one wave per 32x32 output tile (the whole op is <1 % of a forward).
// ---------------------------------------------------------------------------
// qkv [N][HW][3C]; head hd of image b: q / k / v start at channel qo / ko / vo (attn_offsets), `ch` channels each
__device__ __forceinline__ void attn_offsets(int C, int heads, int hd, int& qo, int& ko, int& vo) {
  const int ch = C / heads;
  if (heads > 1) { qo = hd * 3 * ch; ko = qo + ch; vo = qo + 2 * ch; }   // QKVAttentionLegacy: [head][q|k|v][ch]
  else { qo = 0; ko = C; vo = 2 * C; }
}

__global__ void __launch_bounds__(64) attn_scores_kernel(const float* __restrict__ qkv, float* __restrict__ S, int HW, int HWp,
                                                         int C, int heads, float inv_div) {
  const int lane = threadIdx.x, r31 = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32, bh = blockIdx.z, b = bh / heads, hd = bh % heads;
  const int ch = C / heads;
  int qo, ko, vo;
  attn_offsets(C, heads, hd, qo, ko, vo);
  const float* base = qkv + (size_t)b * HW * 3 * C;
  const float* qrow = base + (size_t)min(m0 + r31, HW - 1) * 3 * C + qo + 4 * h;      // A[i = query][k = channel]
  const float* krow = base + (size_t)min(n0 + r31, HW - 1) * 3 * C + ko + 4 * h;      // B[k][j = key] = K[j][k]
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k = 0; k < ch; k += 8) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(qrow + k);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(krow + k);
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s2], bb[s2], acc, 0, 0, 0);
  }
  const int col = n0 + r31;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (row < HW && col < HW) S[((size_t)bh * HW + row) * HWp + col] = acc[i] * inv_div;
  }
}

// rows of pitch HWp >= HW (multiple of 16); the pad columns are written as exact zeros
__global__ void __launch_bounds__(256) softmax_rows_kernel(float* __restrict__ S, int HW, int HWp, size_t rows) {
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  float* r = S + row * HWp;
  float m = -INFINITY;
  for (int i = lane; i < HW; i += 64) m = fmaxf(m, r[i]);
  m = wave_max(m);
  float sum = 0.f;
  for (int i = lane; i < HW; i += 64) { const float e = expf(r[i] - m); r[i] = e; sum += e; }
  sum = wave_sum(sum);
  for (int i = lane; i < HWp; i += 64) r[i] = i < HW ? r[i] / sum : 0.f;
}

__global__ void __launch_bounds__(64) attn_pv_kernel(const float* __restrict__ P, const float* __restrict__ qkv,
                                                     float* __restrict__ O, int HW, int HWp, int C, int heads) {
  const int lane = threadIdx.x, r31 = lane & 31, h = lane >> 5;
  const int ch = C / heads, nblk = ch / 32;
  const int hd = blockIdx.x / nblk, n0 = (blockIdx.x % nblk) * 32, m0 = blockIdx.y * 32, b = blockIdx.z;   // n: channel of the head, m: query
  int qo, ko, vo;
  attn_offsets(C, heads, hd, qo, ko, vo);
  const float* prow = P + ((size_t)(b * heads + hd) * HW + min(m0 + r31, HW - 1)) * HWp + 4 * h;   // A[i = query][k = key]
  const float* vcol = qkv + (size_t)b * HW * 3 * C + vo + n0 + r31;                               // B[k = key][j = channel]
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k = 0; k < HWp; k += 8) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(prow + k);
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      const float bv = vcol[(size_t)min(k + 4 * h + s2, HW - 1) * 3 * C];   // pad keys carry P == 0
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s2], bv, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (row < HW) O[((size_t)b * HW + row) * C + hd * ch + n0 + r31] = acc[i];   // a.reshape(bs, heads*ch, T): head-major channels
  }
}

// S: scratch of attn_scratch_floats(N, HW, heads) floats
size_t attn_scratch_floats(int N, int HW, int heads) { return (size_t)N * heads * HW * ((HW + 15) / 16 * 16); }

// ---- bf16 mode (activations stored as bf16): Q K^T and P V on v_mfma_f32_32x32x16_bf16 -- the "MFMA bf16 QK^T.V contraction" of
// BASELINE.json's north_star, for the siblings that do attend (ddpm_modules/unet.py:99, tesr_modules).  Scores and the softmax stay
// fp32; P is rounded to bf16 as it enters the second product; O is stored as bf16.
// PREC: PREC_BF16 or PREC_F16 (the f16 mode's twin: the same kernels on v_mfma_f32_32x32x16_f16, O stored as f16)
typedef __bf16 bfrag8 __attribute__((ext_vector_type(8)));
template <int PREC>
__global__ void __launch_bounds__(64) attn_scores_bf16_kernel(const unsigned short* __restrict__ qkv, float* __restrict__ S, int HW, int HWp,
                                                              int C, int heads, float inv_div) {
  const int lane = threadIdx.x, r31 = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32, bh = blockIdx.z, b = bh / heads, hd = bh % heads;
  const int ch = C / heads;
  int qo, ko, vo;
  attn_offsets(C, heads, hd, qo, ko, vo);
  const unsigned short* base = qkv + (size_t)b * HW * 3 * C;
  const unsigned short* qrow = base + (size_t)min(m0 + r31, HW - 1) * 3 * C + qo + 8 * h;   // A[i = query][k = 8 h + j]
  const unsigned short* krow = base + (size_t)min(n0 + r31, HW - 1) * 3 * C + ko + 8 * h;   // B[k = 8 h + j][j = key]
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k = 0; k < ch; k += 16) {
    const uint4 a = *reinterpret_cast<const uint4*>(qrow + k);
    const uint4 bb = *reinterpret_cast<const uint4*>(krow + k);
    acc = mfma32_k16<PREC>(a, bb, acc);
  }
  const int col = n0 + r31;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (row < HW && col < HW) S[((size_t)bh * HW + row) * HWp + col] = acc[i] * inv_div;
  }
}

template <int PREC>
__global__ void __launch_bounds__(64) attn_pv_bf16_kernel(const float* __restrict__ P, const unsigned short* __restrict__ qkv,
                                                          unsigned short* __restrict__ O, int HW, int HWp, int C, int heads) {
  const int lane = threadIdx.x, r31 = lane & 31, h = lane >> 5;
  const int ch = C / heads, nblk = ch / 32;
  const int hd = blockIdx.x / nblk, n0 = (blockIdx.x % nblk) * 32, m0 = blockIdx.y * 32, b = blockIdx.z;
  int qo, ko, vo;
  attn_offsets(C, heads, hd, qo, ko, vo);
  const float* prow = P + ((size_t)(b * heads + hd) * HW + min(m0 + r31, HW - 1)) * HWp + 8 * h;   // A[i = query][k = key 8 h + j]
  const unsigned short* vcol = qkv + (size_t)b * HW * 3 * C + vo + n0 + r31;                       // B[k = key][j = channel]
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k = 0; k < HWp; k += 16) {                       // HWp is a multiple of 16; pad keys carry P == 0
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(prow + k), p1 = *reinterpret_cast<const f32x4*>(prow + k + 4);
    uint4 a, bv;                                            // probabilities (in [0, 1]) rounded to the mode's format; V as stored
    {
      const uint2 lo = stage4_16<PREC>(p0), hi = stage4_16<PREC>(p1);
      a = uint4{lo.x, lo.y, hi.x, hi.y};
    }
    unsigned short vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) vv[j] = vcol[(size_t)min(k + 8 * h + j, HW - 1) * 3 * C];
    bv = uint4{(unsigned)vv[0] | ((unsigned)vv[1] << 16), (unsigned)vv[2] | ((unsigned)vv[3] << 16), (unsigned)vv[4] | ((unsigned)vv[5] << 16),
               (unsigned)vv[6] | ((unsigned)vv[7] << 16)};
    acc = mfma32_k16<PREC>(a, bv, acc);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (row < HW) O[((size_t)b * HW + row) * C + hd * ch + n0 + r31] = PREC == PREC_F16 ? f32_to_f16_bits(acc[i]) : f32_to_bf16_bits(acc[i]);
  }
}

hipError_t launch_attn_probs(const float* qkv, float* S, int N, int HW, int C, int heads, hipStream_t s) {
  if (heads < 1 || C % heads || (C / heads) % 32) return hipErrorInvalidValue;
  const int HWp = (HW + 15) / 16 * 16, ch = C / heads;
  const float inv_div = 1.0f / sqrtf((float)ch);
  const size_t rows = (size_t)N * heads * HW;
  const dim3 gs((HW + 31) / 32, (HW + 31) / 32, N * heads);
  hipLaunchKernelGGL(attn_scores_kernel, gs, dim3(64), 0, s, qkv, S, HW, HWp, C, heads, inv_div);
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, S, HW, HWp, rows);
  return hipGetLastError();
}

hipError_t launch_self_attention(const float* qkv, float* S, float* O, int N, int HW, int C, int heads, hipStream_t s, int act_bf16) {
  if (heads < 1 || C % heads || (C / heads) % 32) return hipErrorInvalidValue;
  const int HWp = (HW + 15) / 16 * 16, ch = C / heads;
  // QKVAttentionLegacy scales q and k by ch^-1/4 each (gdp_modules/unet.py:480-483); SelfAttention divides by sqrt(C)
  const float inv_div = 1.0f / sqrtf((float)ch);
  const size_t rows = (size_t)N * heads * HW;
  const dim3 gs((HW + 31) / 32, (HW + 31) / 32, N * heads), gp(C / 32, (HW + 31) / 32, N);
  if (act_bf16) {   // 1 bf16, 2 f16
    const unsigned short* q16 = reinterpret_cast<const unsigned short*>(qkv);
    if (act_bf16 == 2) hipLaunchKernelGGL(attn_scores_bf16_kernel<PREC_F16>, gs, dim3(64), 0, s, q16, S, HW, HWp, C, heads, inv_div);
    else hipLaunchKernelGGL(attn_scores_bf16_kernel<PREC_BF16>, gs, dim3(64), 0, s, q16, S, HW, HWp, C, heads, inv_div);
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, S, HW, HWp, rows);
    if (act_bf16 == 2) hipLaunchKernelGGL(attn_pv_bf16_kernel<PREC_F16>, gp, dim3(64), 0, s, S, q16, reinterpret_cast<unsigned short*>(O), HW, HWp, C, heads);
    else hipLaunchKernelGGL(attn_pv_bf16_kernel<PREC_BF16>, gp, dim3(64), 0, s, S, q16, reinterpret_cast<unsigned short*>(O), HW, HWp, C, heads);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(attn_scores_kernel, gs, dim3(64), 0, s, qkv, S, HW, HWp, C, heads, inv_div);
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, S, HW, HWp, rows);
  hipLaunchKernelGGL(attn_pv_kernel, gp, dim3(64), 0, s, S, qkv, O, HW, HWp, C, heads);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// materialised resampling of the GDP up/down ResBlocks
// ---------------------------------------------------------------------------
// PREC: PREC_F16X3 = fp32 activations (f32 and f16x3 modes), PREC_BF16 = bf16 activations
template <int PREC>
__global__ void __launch_bounds__(256) pool2_kernel(const float* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                                    float* __restrict__ out, int H, int W, int cq, size_t total) {
  using IO = ActIO<PREC>;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // over [N][H/2][W/2][cq]
  if (i >= total) return;
  const int c4 = (int)(i % cq);
  size_t r = i / cq;
  const int Wo = W >> 1, Ho = H >> 1;
  const int ox = (int)(r % Wo);
  r /= Wo;
  const int oy = (int)(r % Ho);
  const size_t n = r / Ho;
  f32x4 a = {1.f, 1.f, 1.f, 1.f}, b = {0.f, 0.f, 0.f, 0.f};
  if (sc) {
    a = *reinterpret_cast<const f32x4*>(sc + (n * cq + c4) * 4);
    b = *reinterpret_cast<const f32x4*>(sh + (n * cq + c4) * 4);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      f32x4 v = IO::widen(IO::load4(x, (((n * H + 2 * oy + dy) * W + 2 * ox + dx) * cq + c4) * 4));
      if (sc) {
        v = v * a + b;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = silu_fast(v[e]);
      }
      acc += v;
    }
  acc = acc * 0.25f;
  if (prec_is16(PREC)) {
    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(out) + i * 4) = pack4_16<PREC>(acc);
  } else {
    *reinterpret_cast<f32x4*>(out + i * 4) = acc;
  }
}

hipError_t launch_pool2(const float* x, const float* gn_scale, const float* gn_shift, float* out, int N, int H, int W, int C,
                        hipStream_t s, int act_bf16) {
  if ((C & 3) || (H & 1) || (W & 1)) return hipErrorInvalidValue;
  const size_t total = (size_t)N * (H >> 1) * (W >> 1) * (C >> 2);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (act_bf16 == 2) hipLaunchKernelGGL(pool2_kernel<PREC_F16>, grid, dim3(256), 0, s, x, gn_scale, gn_shift, out, H, W, C >> 2, total);
  else if (act_bf16) hipLaunchKernelGGL(pool2_kernel<PREC_BF16>, grid, dim3(256), 0, s, x, gn_scale, gn_shift, out, H, W, C >> 2, total);
  else hipLaunchKernelGGL(pool2_kernel<PREC_F16X3>, grid, dim3(256), 0, s, x, gn_scale, gn_shift, out, H, W, C >> 2, total);
  return hipGetLastError();
}

template <typename Q>   // Q: four consecutive channels as stored (f32x4, or uint2 = 4 x bf16)
__global__ void __launch_bounds__(256) upsample2_kernel(const Q* __restrict__ x, Q* __restrict__ out, int H, int W, int cq,
                                                        size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // over [N][2H][2W][cq]
  if (i >= total) return;
  const int c4 = (int)(i % cq);
  size_t r = i / cq;
  const int ox = (int)(r % (2 * W));
  r /= (2 * W);
  const int oy = (int)(r % (2 * H));
  const size_t n = r / (2 * H);
  out[i] = x[((n * H + (oy >> 1)) * W + (ox >> 1)) * cq + c4];
}

hipError_t launch_upsample2(const float* x, float* out, int N, int H, int W, int C, hipStream_t s, int act_bf16) {
  if (C & 3) return hipErrorInvalidValue;
  const size_t total = (size_t)N * 2 * H * 2 * W * (C >> 2);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (act_bf16)
    hipLaunchKernelGGL(upsample2_kernel<uint2>, grid, dim3(256), 0, s, reinterpret_cast<const uint2*>(x), reinterpret_cast<uint2*>(out), H, W, C >> 2, total);
  else
    hipLaunchKernelGGL(upsample2_kernel<f32x4>, grid, dim3(256), 0, s, reinterpret_cast<const f32x4*>(x), reinterpret_cast<f32x4*>(out), H, W, C >> 2, total);
  return hipGetLastError();
}

hipError_t kernels_init() {
  hipError_t e;
#define X(KS_, ST_, UP_, KC_, BN_, WM_) \
  if ((e = init_conv_t<KS_, ST_, UP_, KC_, BN_, WM_>()) != hipSuccess) return e;
  FDSR_CONV_INSTANCES(X)
#undef X
  return hipSuccess;
}

}  // namespace fdsr
