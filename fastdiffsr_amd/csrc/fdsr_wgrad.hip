// Convolution weight-gradient kernels for gfx950 (declared in fdsr_train.h): the exact fp32 MFMA form and the three split-f16
// ("f16x3") forms, the fold of their slices, the slice plan and the scratch sizing that both come from, the launchers.
//   wgrad_kernel      exact fp32, 4 waves
//   wgrad_h_kernel    f16x3, 4 waves (stride 2, 1x1, concat seams, tensors of 4 GiB or more)
//   wgrad_h8_kernel   f16x3, 8 waves, double-buffered (gn_plain layers, wgrad_form=2)
//   wgrad_h8i_kernel  f16x3, 8 waves, staging inside the MFMA rows (almost all of the work)
// Written once: the workgroup's block and slice (WgBlock), the 4-wave kernels' prefetch registers and activation, the 8-wave
// kernels' tile set-up, split and MFMA row, the slice plan behind launchers and scratch sizing.  The remaining per-kernel
// staging, operand addressing and epilogues stay in the kernels: hoisted into functions they compile to different code.
// Every reduction is ordered: a step is bitwise reproducible.
#include "fdsr_train.h"
#include "fdsr_train_dev.h"
#include "fdsr_conv_dev.h"

#include <algorithm>
#include <climits>

namespace fdsr {

// ---------------------------------------------------------------------------
// shared by all four kernels
// ---------------------------------------------------------------------------
// Every workgroup owns one (64 output channels x 64 input channels) block of dW, all taps, over a slice of the output tiles;
// slices write their blocks to scratch [sl][cb][ib][t][64 co][64 ci], wgrad_fold_kernel sums the slices in order.
struct WgBlock {
  int sl, ib, cb, co0, ci0;      // slice, input- and output-channel block and their first channels
  int Cin, tilesX, tilesY;
  int t0, t1;                    // the slice's tiles
  int Hsrc, Wsrc;                // grid the conv taps walk on
};

__device__ __forceinline__ void wg_block(WgBlock& k, const WgradParams& p, int nslices, int ncb, int nib, int TH, int TW, bool up) {
  (void)ncb;
  int b = blockIdx.x;
  k.sl = b % nslices;  b /= nslices;
  k.ib = b % nib;  b /= nib;
  k.cb = b;                                                // < ncb
  k.co0 = k.cb * 64;
  k.ci0 = k.ib * 64;
  k.Cin = p.C0 + p.C1;
  k.tilesX = (p.Wout + TW - 1) / TW;
  k.tilesY = (p.Hout + TH - 1) / TH;
  const int ntiles = p.N * k.tilesX * k.tilesY;
  k.t0 = (int)((long)k.sl * ntiles / nslices);
  k.t1 = (int)((long)(k.sl + 1) * ntiles / nslices);
  k.Hsrc = up ? p.Hout : p.Hin;
  k.Wsrc = up ? p.Wout : p.Win;
}

__device__ __forceinline__ float* wg_scratch_block(const WgradParams& p, const WgBlock& k, int ncb, int nib, int T) {
  return p.scratch + ((((size_t)k.sl * ncb + k.cb) * nib + k.ib) * T) * 4096;
}

// ---------------------------------------------------------------------------
// the 4-wave kernels' staging (wgrad_kernel, wgrad_h_kernel)
// ---------------------------------------------------------------------------
// 4x16-pixel tiles (2x16 at stride 2): 47 KB of LDS per fp32 workgroup, so two workgroups share a CU and one's staging runs
// beside the other's MFMAs (an 8x16 tile needs 84 KB: one workgroup per CU, nothing overlaps)
template <int KS_, int STRIDE_, bool UP_>
struct WgTile4 {
  static constexpr int KS = KS_, STRIDE = STRIDE_, PAD = KS_ / 2;
  static constexpr bool UP = UP_;
  static constexpr int TH = STRIDE_ == 2 ? 2 : 4, TW = 16, T = KS_ * KS_;
  static constexpr int HH = (TH - 1) * STRIDE_ + KS_, HWD = (TW - 1) * STRIDE_ + KS_, NPIX = HH * HWD;
};

// The NEXT tile's dy tile and raw input halo, prefetched into registers while the MFMAs of the current one run (the activation
// is applied when the registers are stored to LDS): thread -> (channel quad q = tid & 15, pixels i*16 + prow, prow = tid >> 4).
// (The prefetch itself is a lambda in each kernel: as a shared function it compiles to different address arithmetic.)
template <class Cfg>
struct WgRegs {
  static constexpr int NDY = Cfg::TH * Cfg::TW * 16 / 256, NIN = (Cfg::NPIX * 16 + 255) / 256;
  f32x4 dy[NDY], in[NIN], sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  unsigned mask[NIN];
  bool ok[NIN];
};

// GroupNorm-apply, Swish and Dropout of one quad, as the fp32 forward stages it
__device__ __forceinline__ f32x4 activate(f32x4 v, f32x4 sc, f32x4 sh, unsigned mask, const WgradParams& p) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float u = fmaf(v[e], sc[e], sh[e]);
    v[e] = p.gn_plain ? u : u * sigmoid_f(u);
  }
  if (p.drop_mask) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((mask >> (8 * e)) & 0xffu) ? v[e] * p.drop_scale : 0.f;
  }
  return v;
}

// halo quad i as it goes to LDS: the conv zero-pads the ACTIVATED tensor
template <class Cfg>
__device__ __forceinline__ f32x4 wg_halo_quad(const WgRegs<Cfg>& r, int i, const WgradParams& p) {
  f32x4 v = r.in[i];
  if (r.ok[i] && p.gn_scale) v = activate(v, r.sc, r.sh, r.mask[i], p);
  return v;
}

// ---------------------------------------------------------------------------
// convolution weight gradient: exact fp32 on v_mfma_f32_32x32x2_f32
// ---------------------------------------------------------------------------
// Workgroup = 4 waves.  Per tile the dy tile [64 px][64 co] and the activated input halo
// [(4-1)*S+KS x (16-1)*S+KS px][64 ci] are staged in LDS (GroupNorm-apply + Swish fused, as the forward does);
// wave (wc, wi) then accumulates, for every tap, dW[32 co][32 ci] += dy^T (32 x 2 px) * a (2 px x 32) over the
// 32 pixel pairs: 9 accumulator tiles (144 VGPRs) per wave.
template <int KS, int STRIDE, bool UP>
struct WgCfg : WgTile4<KS, STRIDE, UP> {
  using G = WgTile4<KS, STRIDE, UP>;
  static constexpr int ROW = 64 + 4;                       // floats per staged pixel (pad: conflict-free 32-lane rows)
  static constexpr int LDS_BYTES = (G::TH * G::TW + G::NPIX) * ROW * 4;
};

template <int KS, int STRIDE, bool UP>
__global__ void __launch_bounds__(256) wgrad_kernel(const WgradParams p, const int nslices, const int ncb, const int nib) {
  using Cfg = WgCfg<KS, STRIDE, UP>;
  constexpr int TH = Cfg::TH, TW = Cfg::TW, T = Cfg::T, HWD = Cfg::HWD, NPIX = Cfg::NPIX, ROW = Cfg::ROW;
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  float* sDy = wsm;                       // [TH*TW][ROW]
  float* sIn = wsm + TH * TW * ROW;       // [NPIX][ROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wc = wave & 1, wi = wave >> 1;                 // 32-channel halves of the (co, ci) block
  WgBlock k;
  wg_block(k, p, nslices, ncb, nib, TH, TW, UP);

  f32x16 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  const int r31 = lane & 31, kh = lane >> 5;
  const int q = tid & 15, prow = tid >> 4;
  WgRegs<Cfg> r;
  constexpr int PAD = Cfg::PAD;
  auto prefetch = [&](int tile) {
    int tt = tile;
    const int tx = tt % k.tilesX;  tt /= k.tilesX;
    const int ty = tt % k.tilesY;
    const int n = tt / k.tilesY;
    const int oy0 = ty * TH, ox0 = tx * TW;
#pragma unroll
    for (int i = 0; i < WgRegs<Cfg>::NDY; ++i) {
      const int px = i * 16 + prow;
      const int oy = oy0 + px / TW, ox = ox0 + px % TW, co = k.co0 + q * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (oy < p.Hout && ox < p.Wout && co < p.Cout_s)
        v = *reinterpret_cast<const f32x4*>(p.dy + ((size_t)(n * p.Hout + oy) * p.Wout + ox) * p.Cout_s + co);
      r.dy[i] = v;
    }
    const int c = k.ci0 + q * 4;
    if (p.gn_scale && c < k.Cin) {
      r.sc = *reinterpret_cast<const f32x4*>(p.gn_scale + (size_t)n * k.Cin + c);
      r.sh = *reinterpret_cast<const f32x4*>(p.gn_shift + (size_t)n * k.Cin + c);
    }
#pragma unroll
    for (int i = 0; i < WgRegs<Cfg>::NIN; ++i) {
      const int hp = i * 16 + prow;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      unsigned m = 0x01010101u;
      bool ok = false;
      if (hp < NPIX) {
        const int hy = hp / HWD, hx = hp % HWD;
        const int iy = oy0 * STRIDE - PAD + hy, ix = ox0 * STRIDE - PAD + hx;
        if (iy >= 0 && iy < k.Hsrc && ix >= 0 && ix < k.Wsrc && c < k.Cin) {
          const int sy = UP ? (iy >> 1) : iy, sx = UP ? (ix >> 1) : ix;
          const float* xs; int Cs, cc;
          if (c < p.C0) { xs = p.x0; Cs = p.C0; cc = c; } else { xs = p.x1; Cs = p.C1; cc = c - p.C0; }
          const size_t o = ((size_t)(n * p.Hin + sy) * p.Win + sx) * Cs + cc;
          v = *reinterpret_cast<const f32x4*>(xs + o);
          if (p.drop_mask) m = *reinterpret_cast<const unsigned*>(p.drop_mask + o);   // dropout sits between the Swish and the conv (C1 == 0 there)
          ok = true;
        }
      }
      r.in[i] = v;
      r.mask[i] = m;
      r.ok[i] = ok;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < WgRegs<Cfg>::NDY; ++i) *reinterpret_cast<f32x4*>(sDy + (i * 16 + prow) * ROW + q * 4) = r.dy[i];
#pragma unroll
    for (int i = 0; i < WgRegs<Cfg>::NIN; ++i) {
      const int hp = i * 16 + prow;
      if (hp >= NPIX) continue;
      *reinterpret_cast<f32x4*>(sIn + hp * ROW + q * 4) = wg_halo_quad(r, i, p);
    }
  };
  if (k.t0 < k.t1) prefetch(k.t0);
  for (int tile = k.t0; tile < k.t1; ++tile) {
    __syncthreads();                                       // the previous tile's reads are done
    store();
    __syncthreads();
    if (tile + 1 < k.t1) prefetch(tile + 1);                 // in flight under the MFMAs below
    // ---- pixel pairs: A = dy^T (lane: co = r31, pixel kh of the pair), B = a shifted by the tap ----
#pragma unroll 2
    for (int pp = 0; pp < TH * TW / 2; ++pp) {
      // the pair = pixels (x, x + 8) of one tile row: their LDS rows are 8*ROW floats apart = 32 banks,
      // so the two half-waves read disjoint banks
      const int py = pp >> 3, pxx = (pp & 7) + 8 * kh;
      const int px = py * TW + pxx;                         // this lane's pixel of the pair
      const float av = sDy[px * ROW + wc * 32 + r31];
      const float* brow = sIn + ((py * STRIDE) * HWD + pxx * STRIDE) * ROW + wi * 32 + r31;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float bv = brow[((t / KS) * HWD + (t % KS)) * ROW];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
      }
    }
  }
  // ---- write this slice's block; D layout: col n = r31 (ci), rows 8*(i/4) + 4*kh + i%4 (co)
  float* dst = wg_scratch_block(p, k, ncb, nib, T);
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;      // co within the wave's 32
      dst[(size_t)t * 4096 + (wc * 32 + row) * 64 + wi * 32 + r31] = acc[t][i];
    }
}

// dw[co][ci][t] = sum over slices (in order) of scratch[sl][cb][ib][t][co%64][ci%64]
__global__ void __launch_bounds__(256) wgrad_fold_kernel(const float* __restrict__ scratch, float* __restrict__ dw, int Cout, int Cin_real,
                                                         int T, int nslices, int ncb, int nib, size_t total) {
  // One workgroup folds 64 consecutive scratch elements (one row of a 64x64 (co, ci) block of one tap): wave w sums the w-th
  // quarter of the slices in ascending order (256 contiguous bytes per slice and wave), the four partial sums are added in
  // wave order -- a fixed association, fp64 -- and the row goes to the checkpoint layout [Cout][Cin][tap].
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t e = (size_t)blockIdx.x * 64 + lane;              // over [cb][ib][t][co & 63][ci & 63]
  const size_t stride = (size_t)ncb * nib * T * 4096;
  const int s0 = w * nslices / 4, s1 = (w + 1) * nslices / 4;
  const float* src = scratch + e;
  double a = 0.0;
  int sl = s0;
  for (; sl + 8 <= s1; sl += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(sl + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += (double)v[u];
  }
  for (; sl < s1; ++sl) a += (double)src[(size_t)sl * stride];
  part[w][lane] = a;
  __syncthreads();
  if (w == 0) {
    const double r = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    size_t q = e;
    const int ci = (int)(q & 63);  q >>= 6;
    const int co = (int)(q & 63);  q >>= 6;
    const int t = (int)(q % T);  q /= T;
    const int ib = (int)(q % nib), cb = (int)(q / nib);
    const int gco = cb * 64 + co, gci = ib * 64 + ci;
    if (gco < Cout && gci < Cin_real) dw[((size_t)gco * Cin_real + gci) * T + t] = (float)r;
  }
}

// ---------------------------------------------------------------------------
// convolution weight gradient, split-f16 ("f16x3") form: v_mfma_f32_32x32x16_f16, three MFMAs per product
// (hi*hi + hi*lo + lo*hi of dy = dh + dl and a = ah + al), fp32 accumulation, fp64 fold of the slices.
// ---------------------------------------------------------------------------
// Pixels are the K dimension and both operands live in HBM pixel-major (NHWC): the MFMA wants, per lane, 8 consecutive
// PIXELS of one channel.  The tiles are staged as plain [pixel][64 channels] f16 images (hi plane, lo plane; coalesced
// loads, 8-byte LDS writes) and read with gfx950's transposing LDS read (ds_read_b64_tr_b16: a 16-lane group fetches a
// 4-pixel x 16-channel block and every lane receives one channel's 4 pixels), two reads per operand half.  A tap only
// changes the FIRST ROW of the B block, so there is no alignment problem and no shifted copy.  Rows are 128 B; the two
// 64-byte halves of a row are swapped on rows with bit 1 set, which makes the 4-row blocks bank-conflict free.
typedef short ts4 __attribute__((ext_vector_type(4)));

template <int KS, int STRIDE, bool UP>
struct WgHCfg : WgTile4<KS, STRIDE, UP> {
  using G = WgTile4<KS, STRIDE, UP>;
  static constexpr int PLANE_DY = G::TH * G::TW * 128, PLANE_IN = G::NPIX * 128;     // bytes per plane
  static constexpr int LDS_BYTES = 2 * PLANE_DY + 2 * PLANE_IN;
};

__device__ __forceinline__ int tr_img_off(int row, int col) {   // byte offset of (pixel row, channel col) inside a plane
  return row * 128 + ((col ^ (((row >> 1) & 1) << 5)) << 1);
}

__device__ __forceinline__ h8 tr_frag(const unsigned char* plane, int row0, int row_step, int col) {
  // 8 k-values of this lane: rows row0 + {0..3} * row_step (first read) and row0 + {4..7} * row_step (second read);
  // lane 4q+p of its 16-lane group supplies the address of row q, columns col .. col+3 (col already includes 4p)
  typedef ts4 __attribute__((address_space(3))) * lds_ts4;
  const int q = (threadIdx.x >> 2) & 3;
  const ts4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ts4)(plane + tr_img_off(row0 + q * row_step, col)));
  const ts4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ts4)(plane + tr_img_off(row0 + (4 + q) * row_step, col)));
  typedef short ts8 __attribute__((ext_vector_type(8)));
  const ts8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(h8, v);
}

template <int KS, int STRIDE, bool UP>
__global__ void __launch_bounds__(256, 2) wgrad_h_kernel(const WgradParams p, const int nslices, const int ncb, const int nib) {
  using Cfg = WgHCfg<KS, STRIDE, UP>;
  constexpr int TH = Cfg::TH, TW = Cfg::TW, T = Cfg::T, HWD = Cfg::HWD, NPIX = Cfg::NPIX;
  extern __shared__ __attribute__((aligned(16))) unsigned char wsh[];
  unsigned char* sDyH = wsh;
  unsigned char* sDyL = wsh + Cfg::PLANE_DY;
  unsigned char* sInH = wsh + 2 * Cfg::PLANE_DY;
  unsigned char* sInL = sInH + Cfg::PLANE_IN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wc = wave & 1, wi = wave >> 1;
  WgBlock k;
  wg_block(k, p, nslices, ncb, nib, TH, TW, UP);

  f32x16 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  const int q4 = tid & 15, prow = tid >> 4;
  WgRegs<Cfg> r;
  constexpr int PAD = Cfg::PAD;
  auto prefetch = [&](int tile) {                          // as in wgrad_kernel
    int tt = tile;
    const int tx = tt % k.tilesX;  tt /= k.tilesX;
    const int ty = tt % k.tilesY;
    const int n = tt / k.tilesY;
    const int oy0 = ty * TH, ox0 = tx * TW;
#pragma unroll
    for (int i = 0; i < WgRegs<Cfg>::NDY; ++i) {
      const int px = i * 16 + prow;
      const int oy = oy0 + px / TW, ox = ox0 + px % TW, co = k.co0 + q4 * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (oy < p.Hout && ox < p.Wout && co < p.Cout_s)
        v = *reinterpret_cast<const f32x4*>(p.dy + ((size_t)(n * p.Hout + oy) * p.Wout + ox) * p.Cout_s + co);
      r.dy[i] = v;
    }
    const int c = k.ci0 + q4 * 4;
    if (p.gn_scale && c < k.Cin) {
      r.sc = *reinterpret_cast<const f32x4*>(p.gn_scale + (size_t)n * k.Cin + c);
      r.sh = *reinterpret_cast<const f32x4*>(p.gn_shift + (size_t)n * k.Cin + c);
    }
#pragma unroll
    for (int i = 0; i < WgRegs<Cfg>::NIN; ++i) {
      const int hp = i * 16 + prow;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      unsigned m = 0x01010101u;
      bool ok = false;
      if (hp < NPIX) {
        const int hy = hp / HWD, hx = hp % HWD;
        const int iy = oy0 * STRIDE - PAD + hy, ix = ox0 * STRIDE - PAD + hx;
        if (iy >= 0 && iy < k.Hsrc && ix >= 0 && ix < k.Wsrc && c < k.Cin) {
          const int sy = UP ? (iy >> 1) : iy, sx = UP ? (ix >> 1) : ix;
          const float* xs; int Cs, cc;
          if (c < p.C0) { xs = p.x0; Cs = p.C0; cc = c; } else { xs = p.x1; Cs = p.C1; cc = c - p.C0; }
          const size_t o = ((size_t)(n * p.Hin + sy) * p.Win + sx) * Cs + cc;
          v = *reinterpret_cast<const f32x4*>(xs + o);
          if (p.drop_mask) m = *reinterpret_cast<const unsigned*>(p.drop_mask + o);
          ok = true;
        }
      }
      r.in[i] = v;
      r.mask[i] = m;
      r.ok[i] = ok;
    }
  };
  // (the two-step split; the 8-wave kernels' put_split() is the packed form of the same values)
  auto put_split2 = [&](unsigned char* ph, unsigned char* pl, int row, f32x4 v) {
    // hi = rn_f16(clamp(v)), lo = rn_f16(v - hi): 22 mantissa bits (fdsr_conv_h.hip)
    typedef _Float16 h4t __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(v[e], -65504.f, 65504.f);
    const h4t hi = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    const h4t lo = {(_Float16)(v[0] - (float)hi[0]), (_Float16)(v[1] - (float)hi[1]), (_Float16)(v[2] - (float)hi[2]),
                    (_Float16)(v[3] - (float)hi[3])};
    const int off = tr_img_off(row, q4 * 4);
    *reinterpret_cast<h4t*>(ph + off) = hi;
    *reinterpret_cast<h4t*>(pl + off) = lo;
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < WgRegs<Cfg>::NDY; ++i) put_split2(sDyH, sDyL, i * 16 + prow, r.dy[i]);
#pragma unroll
    for (int i = 0; i < WgRegs<Cfg>::NIN; ++i) {
      const int hp = i * 16 + prow;
      if (hp >= NPIX) continue;
      put_split2(sInH, sInL, hp, wg_halo_quad(r, i, p));
    }
  };

  // ---- operand addressing: lane -> (16-lane group g, i = 4q + p); channel column = 32 * wave half + 16 * (g & 1) + 4p,
  //      first pixel of the 8-pixel run = 8 * (g >> 1)
  const int g = lane >> 4, pp4 = lane & 3;
  const int colA = wc * 32 + 16 * (g & 1) + 4 * pp4, colB = wi * 32 + 16 * (g & 1) + 4 * pp4;
  const int k0 = 8 * (g >> 1);

  if (k.t0 < k.t1) prefetch(k.t0);
  for (int tile = k.t0; tile < k.t1; ++tile) {
    __syncthreads();
    store();
    __syncthreads();
    if (tile + 1 < k.t1) prefetch(tile + 1);
#pragma unroll 1
    for (int y = 0; y < TH; ++y) {                          // one K-step = one 16-pixel tile row
      const h8 ah = tr_frag(sDyH, y * TW + k0, 1, colA);
      const h8 al = tr_frag(sDyL, y * TW + k0, 1, colA);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int rb = (y * STRIDE + t / KS) * HWD + k0 * STRIDE + (t % KS);
        const h8 bh = tr_frag(sInH, rb, STRIDE, colB);
        const h8 bl = tr_frag(sInL, rb, STRIDE, colB);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t], 0, 0, 0);
      }
    }
  }
  const int r31 = lane & 31, kh = lane >> 5;
  // ---- write this slice's block; D layout: col n = r31 (ci), rows 8*(i/4) + 4*kh + i%4 (co)
  float* dst = wg_scratch_block(p, k, ncb, nib, T);
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;      // co within the wave's 32
      dst[(size_t)t * 4096 + (wc * 32 + row) * 64 + wi * 32 + r31] = acc[t][i];
    }
}

// ---------------------------------------------------------------------------
// the 8-wave f16x3 kernels (stride 1, 3x3): what wgrad_h8_kernel and wgrad_h8i_kernel share
// ---------------------------------------------------------------------------
// One workgroup per CU (two waves per SIMD): waves 0-3 and 4-7 take the upper and lower four rows of an 8x16-pixel tile of the
// same 64 (co) x 64 (ci) block, so a tile is 128 K-values per barrier, and the tiles are double-buffered in LDS.  The two
// half-tile accumulators are added through LDS at the end (rows 0-3 + rows 4-7, a fixed order), so the scratch slices and
// wgrad_fold_kernel are those of the other forms.
template <int KS_, bool UP_>
struct WgH8Cfg {
  static constexpr int KS = KS_, PAD = KS_ / 2;
  static constexpr bool UP = UP_;
  static constexpr int TH = 8, TW = 16, T = KS_ * KS_;
  static constexpr int HH = TH - 1 + KS_, HWD = TW - 1 + KS_, NPIX = HH * HWD;
  static constexpr int PLANE_DY = TH * TW * 128, PLANE_IN = NPIX * 128;     // bytes per plane
  static constexpr int BUF = 2 * PLANE_DY + 2 * PLANE_IN;                   // one tile: dy hi | dy lo | halo hi | halo lo
  static constexpr int RED = T * 4096 * 4;                                  // the final half-tile reduction
  static constexpr int LDS_BYTES = 2 * BUF > RED ? 2 * BUF : RED;
  static constexpr int LDS_BYTES_INROW = 2 * BUF + 4096;                    // + wgrad_h8i_kernel's dummy slot
  static_assert(LDS_BYTES <= 160 * 1024 && LDS_BYTES_INROW <= 160 * 1024, "LDS budget");
};

__device__ __forceinline__ h8 tr_frag_at(const unsigned char* a) {   // two transposing reads: rows +0..3 and +4..7 of this lane's block
  typedef ts4 __attribute__((address_space(3))) * lds_ts4;
  typedef short ts8 __attribute__((ext_vector_type(8)));
  const ts4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ts4)(a));
  const ts4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ts4)(a + 4 * 128));   // row + 4: same swizzle
  const ts8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(h8, v);
}

// the f16x3 split of a quad (split4_mix, fdsr_conv_dev.h) into the two planes of a staging buffer.  lim = 0 zero-pads.
__device__ __forceinline__ void put_split(unsigned char* ph, unsigned char* pl, f32x4 v, float lim) {
  uint2 hi, lo;
  split4_mix(v, lim, hi, lo);
  *reinterpret_cast<uint2*>(ph) = hi;
  *reinterpret_cast<uint2*>(pl) = lo;
}

// The tile being fetched: its first output pixel and image, and the uniform parts of the 32-bit byte offsets of its loads (dy
// tile origin; halo origin, which may lie before the image: the offsets are modular).  Cs: channels of the concat source.
struct H8At { int toy, tox, tn; unsigned ub_dy, ub_in; };

template <class Cfg>
__device__ __forceinline__ void h8_set_tile(H8At& s, const WgradParams& p, const WgBlock& k, int Cs, int tile) {
  int tt = tile;
  s.tox = (tt % k.tilesX) * Cfg::TW;  tt /= k.tilesX;
  s.toy = (tt % k.tilesY) * Cfg::TH;
  s.tn = tt / k.tilesY;
  s.ub_dy = (unsigned)(((s.tn * p.Hout + s.toy) * p.Wout + s.tox) * p.Cout_s) * 4u;
  s.ub_in = (unsigned)(((s.tn * p.Hin + (Cfg::UP ? s.toy / 2 : s.toy - Cfg::PAD)) * p.Win + (Cfg::UP ? s.tox / 2 : s.tox - Cfg::PAD)) * Cs) * 4u;
}

// one K-step = one 16-pixel row y of this wave group's half tile: 27 MFMAs; the B fragments of tap t+1 are read while the
// MFMAs of tap t run
template <class Cfg>
__device__ __forceinline__ void h8_mfma_row(f32x16 (&acc)[Cfg::T], int baseA, const int (&baseB)[4], const unsigned char* cur, int y) {
  constexpr int KS = Cfg::KS, T = Cfg::T, TW = Cfg::TW, HWD = Cfg::HWD;
  const h8 ah = tr_frag_at(cur + baseA + y * TW * 128);
  const h8 al = tr_frag_at(cur + baseA + y * TW * 128 + Cfg::PLANE_DY);
  h8 bh[2], bl[2];
  bh[0] = tr_frag_at(cur + baseB[(y * HWD) & 3] + y * HWD * 128);
  bl[0] = tr_frag_at(cur + baseB[(y * HWD) & 3] + y * HWD * 128 + Cfg::PLANE_IN);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) {
      const int rr = (y + (t + 1) / KS) * HWD + (t + 1) % KS;      // compile-time part of the LDS row
      bh[(t + 1) & 1] = tr_frag_at(cur + baseB[rr & 3] + rr * 128);
      bl[(t + 1) & 1] = tr_frag_at(cur + baseB[rr & 3] + rr * 128 + Cfg::PLANE_IN);
    }
    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[t & 1], acc[t], 0, 0, 0);
    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[t & 1], acc[t], 0, 0, 0);
    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[t & 1], acc[t], 0, 0, 0);
  }
}

// ---- 8 waves, double-buffered tiles ---------------------------------------------------------------------------------
// The NEXT tile is fetched in two halves: its global loads are issued before the 27 MFMAs of two rows and split / written to
// the other LDS buffer after them (one barrier per tile, the staging VALU of one wave under the MFMAs of its SIMD partner).
template <int KS, bool UP>
__global__ void __launch_bounds__(512, 2) wgrad_h8_kernel(const WgradParams p, const int nslices, const int ncb, const int nib) {
  using Cfg = WgH8Cfg<KS, UP>;
  constexpr int TH = Cfg::TH, TW = Cfg::TW, T = Cfg::T, HH = Cfg::HH, HWD = Cfg::HWD, PAD = KS / 2;
  static_assert(KS == 3, "the half-tile staging below is laid out for the 3x3 halo");
  static_assert((2 * HWD) % 4 == 0 && (4 * HWD) % 4 == 0, "the LDS swizzle must not depend on the tile row");
  extern __shared__ __attribute__((aligned(16))) unsigned char wsh8[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = __builtin_amdgcn_readfirstlane(wave >> 2), wc = wave & 1, wi = (wave >> 1) & 1;
  WgBlock k;
  wg_block(k, p, nslices, ncb, nib, TH, TW, UP);
  const int t0 = k.t0, t1 = k.t1;

  f32x16 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  // ---- staging: thread -> channel quad q4 and pixel (ry, rx) of a 2-row x 16-column strip.  The next tile is fetched in two
  // halves; half h = dy rows 4h+ry and 4h+2+ry, halo rows 4h+ry and 4h+2+ry (columns 0..15), plus the halo rows 8+ry (h = 0) or
  // the two right-hand halo columns (h = 1, threads with prow < 2*HH): every index is a shift or a mask and every LDS address is
  // a lane base + an immediate.  Global addresses are tensor base (uniform) + a 32-bit byte offset = uniform tile offset + the
  // lane's offset inside a tile (modular: the halo origin may lie before the image); lanes outside the image read the tensor's
  // first element instead and are zeroed by the clamp (lim = 0).  The launcher guarantees < 4 GiB tensors.
  const int q4 = tid & 15, prow = tid >> 4, ry = prow >> 4, rx = prow & 15;
  const int cdy = k.co0 + q4 * 4, cin = k.ci0 + q4 * 4;
  const bool src0 = k.ci0 < p.C0;                                      // the 64-channel block lies in one concat source (launcher)
  const char* xs = reinterpret_cast<const char*>(src0 ? p.x0 : p.x1);
  const char* dys = reinterpret_cast<const char*>(p.dy);
  const int Cs = src0 ? p.C0 : p.C1, cc = (src0 ? k.ci0 : k.ci0 - p.C0) + q4 * 4;
  const bool gn = p.gn_scale != nullptr, cin_ok = cin < k.Cin, cdy_ok = cdy < p.Cout_s;
  const bool edge_lane = prow < 2 * HH;
  const int ehy = prow >> 1, ehx = TW + (prow & 1);
  auto lsrc = [&](int h) { return UP ? ((h - 1) >> 1) : h; };         // halo coordinate -> source coordinate, lane part
  const unsigned o_dy = (unsigned)((ry * p.Wout + rx) * p.Cout_s + cdy) * 4u;
  const unsigned o_main = (unsigned)((lsrc(ry) * p.Win + lsrc(rx)) * Cs + cc) * 4u;
  const unsigned o_edge = (unsigned)((lsrc(ehy) * p.Win + lsrc(ehx)) * Cs + cc) * 4u;
  const int st_dy = tr_img_off(prow, q4 * 4);                        // + k * 32 rows
  const int st_in = tr_img_off(ry * HWD + rx, q4 * 4);               // + kk * 2 * HWD rows; relative to the halo planes (store_half adds 2 * PLANE_DY)
  const int st_edge = tr_img_off(ehy * HWD + ehx, q4 * 4);
  const unsigned row_dy = (unsigned)(p.Wout * p.Cout_s) * 4u, row_in = (unsigned)(p.Win * Cs) * 4u;   // bytes per image row
  constexpr int NPV = 5;            // registers of one half: 2 dy, 2 halo strips, 1 extra
  f32x4 pv[NPV], nsc = {1.f, 1.f, 1.f, 1.f}, nsh = {0.f, 0.f, 0.f, 0.f};
  unsigned pm[NPV];
  bool pok[NPV];
  H8At at = {0, 0, 0, 0u, 0u};
  auto set_tile = [&](int tile) {
    h8_set_tile<Cfg>(at, p, k, Cs, tile);
    if (gn && cin_ok) {
      nsc = *reinterpret_cast<const f32x4*>(p.gn_scale + (size_t)at.tn * k.Cin + cin);
      nsh = *reinterpret_cast<const f32x4*>(p.gn_shift + (size_t)at.tn * k.Cin + cin);
    }
  };
  auto load_dy = [&](int u, int k) {                                  // dy rows 2k + ry
    const bool ok = at.toy + 2 * k + ry < p.Hout && at.tox + rx < p.Wout && cdy_ok;
    const unsigned off = ok ? at.ub_dy + o_dy + 2 * k * row_dy : 0u;
    pv[u] = *reinterpret_cast<const f32x4*>(dys + off);
    pok[u] = ok;
  };
  auto load_in = [&](int u, unsigned o, int rows, int hy, int hx, bool lane_ok) {
    const bool ok = lane_ok && (unsigned)(at.toy - PAD + hy) < (unsigned)k.Hsrc && (unsigned)(at.tox - PAD + hx) < (unsigned)k.Wsrc && cin_ok;
    const unsigned off = ok ? at.ub_in + o + rows * row_in : 0u;
    pv[u] = *reinterpret_cast<const f32x4*>(xs + off);
    if (p.drop_mask) pm[u] = *reinterpret_cast<const unsigned*>(p.drop_mask + (off >> 2));
    pok[u] = ok;
  };
  auto load_half = [&](int h) {
    load_dy(0, 2 * h);
    load_dy(1, 2 * h + 1);
    load_in(2, o_main, UP ? 2 * h : 4 * h, 4 * h + ry, rx, true);
    load_in(3, o_main, UP ? 2 * h + 1 : 4 * h + 2, 4 * h + 2 + ry, rx, true);
    if (h == 0) load_in(4, o_main, UP ? 4 : 8, 8 + ry, rx, true);
    else load_in(4, o_edge, 0, ehy, ehx, edge_lane);
  };
  auto put_in = [&](int u, unsigned char* inH, int off) {
    f32x4 v = pv[u];
    if (gn) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], nsc[e], nsh[e]);
      if (!p.gn_plain) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * __builtin_amdgcn_rcpf(1.0f + __expf(-v[e]));
      }
      if (p.drop_mask) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ((pm[u] >> (8 * e)) & 0xffu) ? v[e] * p.drop_scale : 0.f;
      }
    }
    put_split(inH + off, inH + Cfg::PLANE_IN + off, v, pok[u] ? 65504.f : 0.f);   // lim = 0: the conv zero-pads the ACTIVATED tensor
  };
  auto store_half = [&](int h, unsigned char* buf) {
    unsigned char* inH = buf + 2 * Cfg::PLANE_DY;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int off = st_dy + (2 * h + u) * 32 * 128;
      put_split(buf + off, buf + Cfg::PLANE_DY + off, pv[u], pok[u] ? 65504.f : 0.f);
    }
    put_in(2, inH, st_in + (2 * h) * 2 * HWD * 128);
    put_in(3, inH, st_in + (2 * h + 1) * 2 * HWD * 128);
    if (h == 0) put_in(4, inH, st_in + 4 * 2 * HWD * 128);
    else if (edge_lane) put_in(4, inH, st_edge);
  };

  // ---- operand addressing: lane -> (16-lane group g, q = row inside the 4-row block, p = column quad); channel column =
  // 32 * wave half + 16 * (g & 1) + 4p, first pixel of the 8-pixel run = 8 * (g >> 1).  The swizzle bit of a read is bit 1 of
  // its LDS row = bit 1 of (c2 + q), c2 = the row's compile-time part mod 4: one lane base per c2, immediates for the rest.
  const int g = lane >> 4, pp4 = lane & 3, q = (lane >> 2) & 3;
  const int k0 = 8 * (g >> 1);
  const int colAb = (wc * 32 + 16 * (g & 1) + 4 * pp4) * 2, colBb = (wi * 32 + 16 * (g & 1) + 4 * pp4) * 2;
  const int baseA = (grp * 4 * TW + k0 + q) * 128 + (colAb ^ (((q >> 1) & 1) << 6));
  int baseB[4];
#pragma unroll
  for (int c2 = 0; c2 < 4; ++c2) baseB[c2] = 2 * Cfg::PLANE_DY + (grp * 4 * HWD + k0 + q) * 128 + (colBb ^ ((((c2 + q) >> 1) & 1) << 6));

  auto mfma_row = [&](const unsigned char* cur, int y) { h8_mfma_row<Cfg>(acc, baseA, baseB, cur, y); };

  if (t0 < t1) {
    set_tile(t0);
#pragma unroll
    for (int h = 0; h < 2; ++h) { load_half(h); store_half(h, wsh8); }
  }
  __syncthreads();
  // The two waves of a SIMD (w and w + 4) run the same loop half a phase apart: waves 0-3 issue the MFMAs of two rows and then
  // split the half tile they fetched before them; waves 4-7 split first (a half fetched two rows earlier -- their first half of
  // the tile after next is fetched under the last two rows) and issue their MFMAs after, so one wave's VALU runs under the
  // other's MFMAs and every fetch has two MFMA rows of both waves to land (40 KB in flight per CU).
  if (grp == 0) {
    for (int tile = t0; tile < t1; ++tile) {
      const int curoff = ((tile - t0) & 1) ? Cfg::BUF : 0;
      const unsigned char* cur = wsh8 + curoff;
      unsigned char* nxt = wsh8 + (Cfg::BUF - curoff);
      const bool more = tile + 1 < t1;
      if (more) set_tile(tile + 1);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (more) load_half(h);
        __builtin_amdgcn_sched_barrier(0);
        mfma_row(cur, 2 * h);
        __builtin_amdgcn_sched_barrier(0);
        mfma_row(cur, 2 * h + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (more) store_half(h, nxt);
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }
  } else {
    if (t0 + 1 < t1) { set_tile(t0 + 1); load_half(0); }
    for (int tile = t0; tile < t1; ++tile) {
      const int curoff = ((tile - t0) & 1) ? Cfg::BUF : 0;
      const unsigned char* cur = wsh8 + curoff;
      unsigned char* nxt = wsh8 + (Cfg::BUF - curoff);
      const bool more = tile + 1 < t1;
      if (more) { store_half(0, nxt); load_half(1); }
      __builtin_amdgcn_sched_barrier(0);
      mfma_row(cur, 0);
      __builtin_amdgcn_sched_barrier(0);
      mfma_row(cur, 1);
      __builtin_amdgcn_sched_barrier(0);
      if (more) store_half(1, nxt);
      if (tile + 2 < t1) { set_tile(tile + 2); load_half(0); }
      __builtin_amdgcn_sched_barrier(0);
      mfma_row(cur, 2);
      __builtin_amdgcn_sched_barrier(0);
      mfma_row(cur, 3);
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
    }
  }

  // ---- rows 4-7 (waves 4-7) are added to rows 0-3 through LDS, then one slice goes to the scratch ----
  const int r31 = lane & 31, kh = lane >> 5;
  float* red = reinterpret_cast<float*>(wsh8);
  if (grp == 1) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
        red[t * 4096 + (wc * 32 + row) * 64 + wi * 32 + r31] = acc[t][i];
      }
  }
  __syncthreads();
  if (grp == 0) {
    float* dst = wg_scratch_block(p, k, ncb, nib, T);
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
        const int o = t * 4096 + (wc * 32 + row) * 64 + wi * 32 + r31;
        dst[o] = acc[t][i] + red[o];
      }
  }
}

// ---- the same with the staging INSIDE the MFMA rows --------------------------------------------------------------------
// wgrad_h8_kernel's knock-outs say its split / activate / LDS-write stream costs as much as its MFMAs and overlaps them only
// partly: an in-order wave cannot issue its own VALU while it is blocked in a run of 27 MFMAs.  Here a tile row is ONE basic
// block: the loads of quarter-piece y+1, the 27 MFMAs of row y with their fragment reads, and the split of piece y (fetched a
// whole row earlier, so no wait) -- branch-free (GN / DROP are template parameters, the last tile re-fetches itself, the two
// right-hand halo columns go to a dummy LDS slot on the lanes that do not own one) -- and sched_group_barrier asks for
// 1 MFMA : 5 VALU : 2 LDS reads per gap.  Two piece register sets (y & 1); both wave groups run the same code.
#ifndef WG_IL_VALU
#define WG_IL_VALU 4
#endif
#ifndef WG_IL_DSR
#define WG_IL_DSR 0
#endif
template <bool UP, bool GN, bool DROP>
__global__ void __launch_bounds__(512, 2) wgrad_h8i_kernel(const WgradParams p, const int nslices, const int ncb, const int nib) {
  using Cfg = WgH8Cfg<3, UP>;
  constexpr int KS = 3, TH = Cfg::TH, TW = Cfg::TW, T = Cfg::T, HH = Cfg::HH, HWD = Cfg::HWD, PAD = 1;
  constexpr int DUMMY = 2 * Cfg::BUF;                      // 8 spare bytes per lane-quad above the two buffers (hi), +2 KB (lo)
  extern __shared__ __attribute__((aligned(16))) unsigned char wsh8[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = __builtin_amdgcn_readfirstlane(wave >> 2), wc = wave & 1, wi = (wave >> 1) & 1;
  WgBlock k;
  wg_block(k, p, nslices, ncb, nib, TH, TW, UP);
  const int t0 = k.t0, t1 = k.t1;

  f32x16 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  if (t0 >= t1) return;                                    // (never: slices <= tiles)

  const int q4 = tid & 15, prow = tid >> 4, ry = prow >> 4, rx = prow & 15;
  const int cdy = k.co0 + q4 * 4, cin = k.ci0 + q4 * 4;
  const bool src0 = k.ci0 < p.C0;
  const char* xs = reinterpret_cast<const char*>(src0 ? p.x0 : p.x1);
  const char* dys = reinterpret_cast<const char*>(p.dy);
  const int Cs = src0 ? p.C0 : p.C1, cc = (src0 ? k.ci0 : k.ci0 - p.C0) + q4 * 4;
  const bool cin_ok = cin < k.Cin, cdy_ok = cdy < p.Cout_s;
  const bool edge_lane = prow < 2 * HH;
  const int ehy = prow >> 1, ehx = TW + (prow & 1);
  auto lsrc = [&](int h) { return UP ? ((h - 1) >> 1) : h; };
  const unsigned o_dy = (unsigned)((ry * p.Wout + rx) * p.Cout_s + cdy) * 4u;
  const unsigned o_main = (unsigned)((lsrc(ry) * p.Win + lsrc(rx)) * Cs + cc) * 4u;
  const unsigned o_edge = (unsigned)((lsrc(ehy) * p.Win + lsrc(ehx)) * Cs + cc) * 4u;
  const int st_dy = tr_img_off(prow, q4 * 4);
  const int st_in = 2 * Cfg::PLANE_DY + tr_img_off(ry * HWD + rx, q4 * 4);   // relative to the buffer (wgrad_h8_kernel's are relative to the halo planes:
                                                                             // either kernel changes its instruction stream when moved to the other's convention)
  const int st_edge = 2 * Cfg::PLANE_DY + tr_img_off(ehy * HWD + ehx, q4 * 4);
  const unsigned row_dy = (unsigned)(p.Wout * p.Cout_s) * 4u, row_in = (unsigned)(p.Win * Cs) * 4u;
  f32x4 pv[2][3], nsc = {1.f, 1.f, 1.f, 1.f}, nsh = {0.f, 0.f, 0.f, 0.f};
  f32x4 cs = {0.f, 0.f, 0.f, 0.f};   // this thread's share of the column sums of dy (bias / noise-shift gradients), real tiles only
  bool cs_real = true;
  unsigned pm[2][3];
  bool pok[2][3];
  H8At at = {0, 0, 0, 0u, 0u};
  auto set_tile = [&](int tile) { h8_set_tile<Cfg>(at, p, k, Cs, tile); };
  auto load_gn = [&]() {
    if (GN) {
      const int c = cin_ok ? cin : 0;
      nsc = *reinterpret_cast<const f32x4*>(p.gn_scale + (size_t)at.tn * k.Cin + c);
      nsh = *reinterpret_cast<const f32x4*>(p.gn_shift + (size_t)at.tn * k.Cin + c);
    }
  };
  auto load_in = [&](int set, int u, unsigned o, int rows, int hy, int hx, bool lane_ok) {
    const bool ok = lane_ok && (unsigned)(at.toy - PAD + hy) < (unsigned)k.Hsrc && (unsigned)(at.tox - PAD + hx) < (unsigned)k.Wsrc && cin_ok;
    const unsigned off = ok ? at.ub_in + o + rows * row_in : 0u;
    pv[set][u] = *reinterpret_cast<const f32x4*>(xs + off);
    if (DROP) pm[set][u] = *reinterpret_cast<const unsigned*>(p.drop_mask + (off >> 2));
    pok[set][u] = ok;
  };
  auto load_piece = [&](int set, int j) {                  // quarter j: dy rows 2j+ry, halo rows 2j+ry, + rows 8+ry (j=0) / edge (j=1)
    {
      const bool ok = at.toy + 2 * j + ry < p.Hout && at.tox + rx < p.Wout && cdy_ok;
      const unsigned off = ok ? at.ub_dy + o_dy + 2 * j * row_dy : 0u;
      pv[set][0] = *reinterpret_cast<const f32x4*>(dys + off);
      pok[set][0] = ok;
    }
    load_in(set, 1, o_main, UP ? j : 2 * j, 2 * j + ry, rx, true);
    if (j == 0) load_in(set, 2, o_main, UP ? 4 : 8, 8 + ry, rx, true);
    if (j == 1) load_in(set, 2, o_edge, 0, ehy, ehx, edge_lane);
  };
  auto put_in = [&](int set, int u, unsigned char* buf, int off, int lo_off) {
    f32x4 v = pv[set][u];
    if (GN) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], nsc[e], nsh[e]);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] * __builtin_amdgcn_rcpf(1.0f + __expf(-v[e]));
      if (DROP) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ((pm[set][u] >> (8 * e)) & 0xffu) ? v[e] * p.drop_scale : 0.f;
      }
    }
    put_split(buf + off, buf + off + lo_off, v, pok[set][u] ? 65504.f : 0.f);
  };
  auto store_piece = [&](int set, int j, unsigned char* buf) {
    {
      const bool add = pok[set][0] && cs_real;
#pragma unroll
      for (int e = 0; e < 4; ++e) cs[e] += add ? pv[set][0][e] : 0.f;
    }
    put_split(buf + st_dy + j * 32 * 128, buf + Cfg::PLANE_DY + st_dy + j * 32 * 128, pv[set][0], pok[set][0] ? 65504.f : 0.f);
    put_in(set, 1, buf, st_in + j * 2 * HWD * 128, Cfg::PLANE_IN);
    if (j == 0) put_in(set, 2, buf, st_in + 4 * 2 * HWD * 128, Cfg::PLANE_IN);
    if (j == 1) {                                           // lanes without a halo-edge pixel write a dummy slot (no branch)
      unsigned char* base = edge_lane ? buf + st_edge : wsh8 + DUMMY + (tid & 255) * 8;
      put_in(set, 2, base, 0, edge_lane ? Cfg::PLANE_IN : 2048);
    }
  };

  const int g = lane >> 4, pp4 = lane & 3, q = (lane >> 2) & 3;
  const int k0 = 8 * (g >> 1);
  const int colAb = (wc * 32 + 16 * (g & 1) + 4 * pp4) * 2, colBb = (wi * 32 + 16 * (g & 1) + 4 * pp4) * 2;
  const int baseA = (grp * 4 * TW + k0 + q) * 128 + (colAb ^ (((q >> 1) & 1) << 6));
  int baseB[4];
#pragma unroll
  for (int c2 = 0; c2 < 4; ++c2) baseB[c2] = 2 * Cfg::PLANE_DY + (grp * 4 * HWD + k0 + q) * 128 + (colBb ^ ((((c2 + q) >> 1) & 1) << 6));

  auto mfma_row = [&](const unsigned char* cur, int y) { h8_mfma_row<Cfg>(acc, baseA, baseB, cur, y); };
  auto interleave = [&]() {                                 // the shape asked of the scheduler for a row block
#pragma unroll
    for (int i = 0; i < 27; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // 1 MFMA
#if WG_IL_DSR
      __builtin_amdgcn_sched_group_barrier(0x100, WG_IL_DSR, 0);
#endif
      __builtin_amdgcn_sched_group_barrier(0x002, WG_IL_VALU, 0);    // VALU per MFMA gap
    }
  };

  // prologue: tile t0 staged directly, piece 0 of the next fetch tile in flight
  set_tile(t0);
  load_gn();
#pragma unroll
  for (int j = 0; j < 4; ++j) { load_piece(j & 1, j); store_piece(j & 1, j, wsh8); }
  {
    const int f = t0 + 1 < t1 ? t0 + 1 : t1 - 1;
    set_tile(f);
    load_gn();
    load_piece(0, 0);
  }
  __syncthreads();
  for (int tile = t0; tile < t1; ++tile) {
    const int curoff = ((tile - t0) & 1) ? Cfg::BUF : 0;
    const unsigned char* cur = wsh8 + curoff;
    unsigned char* nxt = wsh8 + (Cfg::BUF - curoff);
    cs_real = tile + 1 < t1;                                 // the last tile re-fetches itself: not summed twice
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      // fetch: piece y+1 of tile+1, or (y = 3) piece 0 of tile+2; convert: piece y of tile+1 (fetched during the previous row)
      if (y == 3) set_tile(tile + 2 < t1 ? tile + 2 : t1 - 1);
      load_piece((y + 1) & 1, (y + 1) & 3);
      mfma_row(cur, y);
      store_piece(y & 1, y, nxt);
      if (y == 3) load_gn();                                 // after the last use of this tile's scale / shift
      interleave();
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  }

  // ---- column sums of dy over this slice (one image or part of one): lanes l, l^16, l^32, l^48 share the channel quad ----
  if (p.colsum_part && k.ib == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      cs[e] += __shfl_xor(cs[e], 16, 64);
      cs[e] += __shfl_xor(cs[e], 32, 64);
    }
    float* cred = reinterpret_cast<float*>(wsh8);           // [wave][64 channels]
    if (lane < 16) *reinterpret_cast<f32x4*>(cred + wave * 64 + lane * 4) = cs;
    __syncthreads();
    if (tid < 64) {
      float a = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) a += cred[w * 64 + tid];
      p.colsum_part[((size_t)k.sl * ncb + k.cb) * 64 + tid] = a;
    }
    __syncthreads();
  }
  const int r31 = lane & 31, kh = lane >> 5;
  float* red = reinterpret_cast<float*>(wsh8);
  if (grp == 1) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
        red[t * 4096 + (wc * 32 + row) * 64 + wi * 32 + r31] = acc[t][i];
      }
  }
  __syncthreads();
  if (grp == 0) {
    float* dst = wg_scratch_block(p, k, ncb, nib, T);
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
        const int o = t * 4096 + (wc * 32 + row) * 64 + wi * 32 + r31;
        dst[o] = acc[t][i] + red[o];
      }
  }
}
// S[n][c] = the slices of image n added in slice order
__global__ void __launch_bounds__(256) colsum_slices_kernel(const float* __restrict__ part, float* __restrict__ S, int K, int ncb, int k) {
  const int c = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (c >= K) return;
  double a = 0.0;
  for (int j0 = 0; j0 < k; j0 += 8) {   // (eight slices per trip, in flight together: as sum_rows_kernel)
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[((size_t)(n * k + min(j0 + u, k - 1)) * ncb + (c >> 6)) * 64 + (c & 63)];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += j0 + u < k ? (double)v[u] : 0.0;
  }
  S[(size_t)n * K + c] = (float)a;
}

// ---------------------------------------------------------------------------
// host: how a launch is sliced, how much scratch that needs, the launchers
// ---------------------------------------------------------------------------
static int wgrad_slices(int ntiles, int ncb, int nib) {    // the 4-wave forms
  const int blocks = ncb * nib;
  int s = (1024 + blocks - 1) / blocks;      // ~4 workgroups per CU in total
  if (s > ntiles) s = ntiles;
  if (s > 512) s = 512;
  return s < 1 ? 1 : s;
}

// The 8-wave forms run at most H8_MAX_SLICES workgroups per (co, ci) block set: two rounds of one workgroup per CU, never a
// straggler third.  Free slicing: that many, at most one per tile.  Image-aligned slicing (the in-row kernel's column sums of
// dy want every slice inside ONE image, so that S[n][c] is a sum of whole slices): k0 or k0 + 1 slices per image.
constexpr int H8_MAX_SLICES = 512;
static int h8_free_slices(int blocks, int ntiles) {
  int s = H8_MAX_SLICES / blocks;
  if (s > ntiles) s = ntiles;
  return s < 1 ? 1 : s;
}
static int h8_aligned_k0(int blocks, int N) {
  const int k0 = H8_MAX_SLICES / (blocks * N);
  return k0 < 1 ? 1 : k0;
}

static int tiles_of(int N, int Hout, int Wout, int TH, int TW) { return N * ((Wout + TW - 1) / TW) * ((Hout + TH - 1) / TH); }
static int tile_rows_4wave(ConvKind kind) { return kind == CONV3_S2 ? WgTile4<3, 2, false>::TH : WgTile4<3, 1, false>::TH; }

// How a weight gradient runs: the kernel form, its grid of (co, ci) blocks and its slices (every slice has a tile: ns <= tiles).
struct WgPlan {
  bool h8, inrow, colsum;        // 8-wave form; with the staging in the MFMA rows; that one also producing the column sums of dy
  int ncb, nib, T, ns, k;        // k: slices per image when colsum
  size_t slice_floats() const { return (size_t)ns * ncb * nib * T * 4096; }
  size_t colsum_floats() const { return colsum ? (size_t)ns * ncb * 64 : 0; }   // the partials, behind the slices
};

static WgPlan wgrad_plan(ConvKind kind, const WgradParams& p, bool f16x3) {
  WgPlan r{false, false, false, (p.Cout + 63) / 64, (p.C0 + p.C1 + 63) / 64, kind == CONV1 ? 1 : 9, 1, 0};
  const int blocks = r.ncb * r.nib;
  r.ns = wgrad_slices(tiles_of(p.N, p.Hout, p.Wout, tile_rows_4wave(kind), 16), r.ncb, r.nib);
  if (!f16x3 || (kind != CONV3_S1 && kind != CONV3_UP)) return r;
  const bool four_wave = g_tun.wgrad_form == 1;   // A/B options (fdsr_debug_option): the 4-wave single-buffer form everywhere,
  const bool plain8 = g_tun.wgrad_form == 2;      // the 8-wave form without the in-row interleave
  const bool no_colsum = !g_tun.wgrad_colsum;
  // the 8-wave forms want a 64-channel block inside one concat source and 32-bit byte offsets; the 4-wave form takes the rest
  const size_t in_px = (size_t)p.N * p.Hin * p.Win, out_px = (size_t)p.N * p.Hout * p.Wout;
  const bool seam = (p.C1 > 0 && (p.C0 & 63) != 0) || in_px * (size_t)(p.C0 > p.C1 ? p.C0 : p.C1) * 4 >= (size_t)g_tun.wgrad_big_bytes ||
                    out_px * (size_t)p.Cout_s * 4 >= (size_t)g_tun.wgrad_big_bytes;
  if (four_wave || seam) return r;
  r.h8 = true;
  r.inrow = !plain8 && !p.gn_plain;
  const int tpi = tiles_of(1, p.Hout, p.Wout, WgH8Cfg<3, false>::TH, WgH8Cfg<3, false>::TW);   // tiles per image
  r.ns = h8_free_slices(blocks, p.N * tpi);
  if (r.inrow && !no_colsum && p.Cout_s <= r.ncb * 64) {
    // slices per image: k0 or k0 + 1, whichever fills whole rounds of 256 workgroups better; within [1, tiles per image]
    const int k0 = h8_aligned_k0(blocks, p.N);
    int best = 0;
    double beff = -1.0;
    for (int k = k0; k <= k0 + 1; ++k) {
      if (k > tpi || p.N * k > H8_MAX_SLICES) continue;
      const long w = (long)blocks * p.N * k;
      const double eff = (double)w / (double)(((w + 255) / 256) * 256);
      if (eff > beff + 1e-9) { beff = eff; best = k; }
    }
    if (best > 0) { r.colsum = true; r.k = best; r.ns = p.N * best; }
  }
  return r;
}

bool wgrad_h_fuses_colsum(ConvKind kind, const WgradParams& p) { return wgrad_plan(kind, p, true).colsum; }

// what launch_wgrad (f16x3: launch_wgrad_h, under the options in force) writes to the scratch for an unconcatenated layer
size_t wgrad_launch_floats(ConvKind kind, int N, int Hout, int Wout, int Cin, int Cout, bool gn_plain, bool f16x3) {
  WgradParams p{};
  p.N = N;  p.Hout = Hout;  p.Wout = Wout;
  p.Hin = kind == CONV3_S2 ? 2 * Hout : kind == CONV3_UP ? (Hout + 1) / 2 : Hout;
  p.Win = kind == CONV3_S2 ? 2 * Wout : kind == CONV3_UP ? (Wout + 1) / 2 : Wout;
  p.C0 = Cin;  p.Cout = p.Cout_s = Cout;  p.gn_plain = gn_plain;
  const WgPlan pl = wgrad_plan(kind, p, f16x3);
  return pl.slice_floats() + pl.colsum_floats();
}

// Room for whatever wgrad_plan may choose for a layer of this geometry, at either precision and under every option: the 4-wave
// slices of these tiles; for the kinds with 8-wave forms, their free slicing and each image-aligned candidate however many tiles
// an image has (capped like the plan's), with the column-sum partials.
size_t wgrad_scratch_floats(ConvKind kind, int N, int Hout, int Wout, int Cin, int Cout) {
  const int T = kind == CONV1 ? 1 : 9;
  const int ncb = (Cout + 63) / 64, nib = (Cin + 63) / 64, blocks = ncb * nib;
  const size_t block_floats = (size_t)blocks * T * 4096;
  size_t need = (size_t)wgrad_slices(tiles_of(N, Hout, Wout, tile_rows_4wave(kind), 16), ncb, nib) * block_floats;
  if (kind == CONV3_S1 || kind == CONV3_UP) {
    int ns = h8_free_slices(blocks, INT_MAX);
    const int k0 = h8_aligned_k0(blocks, N);
    for (int k = k0; k <= k0 + 1; ++k) ns = std::max(ns, (int)std::min<long>((long)N * k, H8_MAX_SLICES));
    need = std::max(need, (size_t)ns * block_floats + (size_t)ns * ncb * 64);
  }
  return need;
}

template <class Kernel>
static void launch_slices(Kernel kernel, int threads, size_t lds, const WgradParams& p, const WgPlan& pl, hipStream_t s) {
  hipLaunchKernelGGL(kernel, dim3(pl.ns * pl.ncb * pl.nib), dim3(threads), lds, s, p, pl.ns, pl.ncb, pl.nib);
}

template <int KS, int STRIDE, bool UP>
static void launch_4wave(bool f16x3, const WgradParams& p, const WgPlan& pl, hipStream_t s) {
  if (f16x3) launch_slices(wgrad_h_kernel<KS, STRIDE, UP>, 256, WgHCfg<KS, STRIDE, UP>::LDS_BYTES, p, pl, s);
  else launch_slices(wgrad_kernel<KS, STRIDE, UP>, 256, WgCfg<KS, STRIDE, UP>::LDS_BYTES, p, pl, s);
}

template <bool UP>
static void launch_8wave(const WgradParams& p, const WgPlan& pl, hipStream_t s) {
  using Cfg = WgH8Cfg<3, UP>;
  if (!pl.inrow) launch_slices(wgrad_h8_kernel<3, UP>, 512, Cfg::LDS_BYTES, p, pl, s);
  else if (!p.gn_scale) launch_slices(wgrad_h8i_kernel<UP, false, false>, 512, Cfg::LDS_BYTES_INROW, p, pl, s);
  else if (!p.drop_mask) launch_slices(wgrad_h8i_kernel<UP, true, false>, 512, Cfg::LDS_BYTES_INROW, p, pl, s);
  else launch_slices(wgrad_h8i_kernel<UP, true, true>, 512, Cfg::LDS_BYTES_INROW, p, pl, s);
}

// the slice kernel wgrad_plan chose, then the folds (the 4-wave tiles of the two precisions are equal, so one plan slices both)
static hipError_t launch_wgrad_as(bool f16x3, ConvKind kind, const WgradParams& p0, hipStream_t s) {
  if ((p0.C0 & 3) || (p0.C1 & 3) || (p0.Cout_s & 3)) return hipErrorInvalidValue;
  const WgPlan pl = wgrad_plan(kind, p0, f16x3);
  WgradParams p = p0;
  p.colsum_part = pl.colsum && p.colsum ? p.scratch + pl.slice_floats() : nullptr;
  if (pl.h8) kind == CONV3_UP ? launch_8wave<true>(p, pl, s) : launch_8wave<false>(p, pl, s);
  else switch (kind) {
    case CONV3_S1: launch_4wave<3, 1, false>(f16x3, p, pl, s); break;
    case CONV3_S2: launch_4wave<3, 2, false>(f16x3, p, pl, s); break;
    case CONV3_UP: launch_4wave<3, 1, true>(f16x3, p, pl, s); break;
    case CONV1: launch_4wave<1, 1, false>(f16x3, p, pl, s); break;   // (f16x3: bandwidth-bound, two small workgroups per CU keep more loads in flight)
    default: return hipErrorInvalidValue;
  }
  const size_t total = (size_t)p.Cout * p.Cin_real * pl.T;
  hipLaunchKernelGGL(wgrad_fold_kernel, dim3((unsigned)(pl.ncb * pl.nib * pl.T * 64)), dim3(256), 0, s, p.scratch, p.dw, p.Cout, p.Cin_real,
                     pl.T, pl.ns, pl.ncb, pl.nib, total);
  if (p.colsum_part)
    hipLaunchKernelGGL(colsum_slices_kernel, dim3((p.Cout_s + 255) / 256, p.N), dim3(256), 0, s, p.colsum_part, p.colsum, p.Cout_s, pl.ncb, pl.k);
  return hipGetLastError();
}

hipError_t launch_wgrad(ConvKind kind, const WgradParams& p, hipStream_t s) { return launch_wgrad_as(false, kind, p, s); }
hipError_t launch_wgrad_h(ConvKind kind, const WgradParams& p, hipStream_t s) { return launch_wgrad_as(true, kind, p, s); }

template <class Kernel>
static hipError_t set_lds_limit(Kernel kernel, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// the 4-wave kernels of one geometry
template <int KS, int STRIDE, bool UP>
static hipError_t init_4wave() {
  const hipError_t e = set_lds_limit(wgrad_kernel<KS, STRIDE, UP>, WgCfg<KS, STRIDE, UP>::LDS_BYTES);
  return e != hipSuccess ? e : set_lds_limit(wgrad_h_kernel<KS, STRIDE, UP>, WgHCfg<KS, STRIDE, UP>::LDS_BYTES);
}
template <bool UP>
static hipError_t init_8wave() {
  using Cfg = WgH8Cfg<3, UP>;
  hipError_t e = set_lds_limit(wgrad_h8_kernel<3, UP>, Cfg::LDS_BYTES);
  if (e == hipSuccess) e = set_lds_limit(wgrad_h8i_kernel<UP, false, false>, Cfg::LDS_BYTES_INROW);
  if (e == hipSuccess) e = set_lds_limit(wgrad_h8i_kernel<UP, true, false>, Cfg::LDS_BYTES_INROW);
  if (e == hipSuccess) e = set_lds_limit(wgrad_h8i_kernel<UP, true, true>, Cfg::LDS_BYTES_INROW);
  return e;
}

hipError_t train_kernels_init() {
  hipError_t e = init_4wave<3, 1, false>();
  if (e == hipSuccess) e = init_4wave<3, 2, false>();
  if (e == hipSuccess) e = init_4wave<3, 1, true>();
  if (e == hipSuccess) e = init_4wave<1, 1, false>();
  if (e == hipSuccess) e = init_8wave<false>();
  if (e == hipSuccess) e = init_8wave<true>();
  return e;
}

}  // namespace fdsr
