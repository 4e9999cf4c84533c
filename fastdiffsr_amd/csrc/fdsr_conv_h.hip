// 16-bit-operand MFMA convolutions for gfx950: v_mfma_f32_32x32x16_{f16,bf16}, fp32 accumulate.
//
// Two arithmetic modes share one kernel:
//   PREC_F16X3  fp32-grade: every fp32 operand x is split on the fly into hi = f16(x) and
//               lo = f16(x - hi) (22 mantissa bits together); the product is formed as
//               hi*hi + hi*lo + lo*hi by three MFMAs into one fp32 accumulator.  Weights are
//               pre-scaled by a power of two (so their lo parts stay normal f16 numbers) and
//               the accumulator is un-scaled in the epilogue.  Measured against the exact-fp32
//               path the 20-step loop differs by ~4e-6, at 3/16 of the fp32-MFMA time.
//   PREC_BF16   one bf16 product (BASELINE config 3; judged on PSNR, not on the 1e-3 bound).
//
// Structure ("weights in registers, pixels from LDS"):
//   * workgroup = 8 wave64 = TH x 32 output pixels x BN = 32*WN output channels
//   * a wave owns 32 output channels (wn) and TH/WM rows of 32 pixels (wm); it keeps the weight
//     fragments of ALL taps of the current 16-channel K-chunk in VGPRs (9 taps x hi/lo x 4
//     VGPRs), loaded straight from L2 in MFMA-fragment order (1 KB contiguous per wave-load), and
//     re-loads tap t's registers for the next chunk right after tap t's last use
//   * the input halo tile of the chunk goes through LDS only: GroupNorm-apply + Swish + hi/lo
//     split are fused into the staging; rows are [16 x hi | 16 x lo | 16 B pad] = 80 B (5 slots,
//     odd) so the 32-pixel-row reads (ds_read_b128) are bank-conflict free with immediate offsets
//   * the halo is double-buffered: chunk k+1 is transformed and written while chunk k is being
//     multiplied; one barrier per chunk
//   * epilogue as in the fp32 kernel (bias + noise-embedding shift + residual, NHWC stores)
#include "fdsr_conv_dev.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace fdsr {

template <int KS, int STRIDE, bool UP, int TH, int WN, int PREC, int KSUB>
struct ConvHCfg {
  static constexpr int TW = 32, NW = 8;
  static constexpr int KC = 16 * KSUB;        // input channels per staged chunk (KSUB > 1 only for 1x1)
  static constexpr int NP = PREC == PREC_F16X3 ? 2 : 1;
  static constexpr int WNP = PREC == PREC_BF16 ? 1 : 2;   // planes per fragment of the weight arena the mode reads (PREC_F16: the f16x3 form, hi plane only)
  static constexpr int ROWB = NP * 32 * KSUB + 16;   // LDS bytes per halo pixel: KSUB x [16 hi | 16 lo] + pad (odd # of 16-B slots)
  static constexpr int PAD = KS / 2;
  static constexpr int HH = (TH - 1) * STRIDE + KS;
  static constexpr int HWD = (TW - 1) * STRIDE + KS;
  static constexpr int NPIX = HH * HWD;
  static constexpr int WM = NW / WN;
  static constexpr int BN = 32 * WN;
  static constexpr int MB = TH / WM;
  static constexpr int NT = 64 * NW;           // threads per workgroup
  static constexpr int Q4 = 4 * KSUB;          // float4 slots per pixel-chunk
  static constexpr int RPP = NT / Q4;          // halo pixels filled per pass
  static constexpr int NIN = (NPIX + RPP - 1) / RPP;
  static constexpr int T = KS * KS * KSUB;     // MFMA k-steps per chunk: spatial taps x 16-channel sub-chunks
  static_assert(KSUB == 1 || KS == 1, "sub-chunking is for 1x1 only");
  static constexpr int BUF_BYTES = (NPIX * ROWB + 15) / 16 * 16;
  static_assert(TH % WM == 0, "TH must be a multiple of WM");
};

#ifdef CONVH_STAMPS
// Diagnostic build only (tools/build_obj_variant.sh <tag> fdsr_conv_h.hip -DCONVH_STAMPS -DCONVH_STAMP_CIN=.. -DCONVH_STAMP_COUT=..
// -DCONVH_STAMP_PREC=..): s_memtime stamps of waves 0 and 7 of the first 256 workgroups of the stride-1 3x3 launches of ONE layer
// shape at the phase boundaries (the last such launch stays); read back by fdsr_diag_convh_stamps (tools/convh_stamps.py).
__device__ unsigned long long g_h_stamps[256][2][64];
#define H_STAMP()                                                                                                  \
  do {                                                                                                             \
    if (stamp_on && si < 64) g_h_stamps[blockIdx.x][wave == 0 ? 0 : 1][si] = __builtin_amdgcn_s_memtime();         \
    ++si;                                                                                                          \
  } while (0)
#else
#define H_STAMP() do {} while (0)
#endif

template <int KS, int STRIDE, bool UP, int TH, int WN, int PREC, int KSUB, bool RIDER = false>
__global__ void __launch_bounds__(512, 2) conv_mfma_h_kernel(const ConvParams p) {
  static_assert(!RIDER || (KS == 3 && STRIDE == 1 && !UP && KSUB == 1), "the rider rides the stride-1 3x3 kernels");
  using Cfg = ConvHCfg<KS, STRIDE, UP, TH, WN, PREC, KSUB>;
  constexpr int TW = Cfg::TW, KC = Cfg::KC, NP = Cfg::NP, ROWB = Cfg::ROWB, PAD = Cfg::PAD, HWD = Cfg::HWD;
  constexpr int NPIX = Cfg::NPIX, WM = Cfg::WM, BN = Cfg::BN, MB = Cfg::MB, RPP = Cfg::RPP, NIN = Cfg::NIN, T = Cfg::T, Q4 = Cfg::Q4, NW = Cfg::NW;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem_h[];
  unsigned char* sBuf0 = smem_h;
  unsigned char* sBuf1 = smem_h + Cfg::BUF_BYTES;
  const int Cin = p.C0 + p.C1;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave % WN, wm = wave / WN;

  const int nco = p.Cout_pad / BN;
  const int tilesX = (p.Wout + TW - 1) / TW, tilesY = (p.Hout + TH - 1) / TH;
  int bid = xcd_block_id(blockIdx.x, gridDim.x);
  const int SK = p.ksplit > 1 ? p.ksplit : 1;
  const int ksi = bid % SK;   // K slice of this workgroup
  bid /= SK;
  const int cot = bid % nco;
  int pt = bid / nco;
  const int tx = pt % tilesX;
  pt /= tilesX;
  const int ty = pt % tilesY;
  const int n = pt / tilesY;
  const int oy0 = ty * TH, ox0 = tx * TW, co0 = cot * BN;

  const bool gn = p.gn_scale != nullptr;
#ifdef CONVH_STAMPS
  int si = 0;
  const bool stamp_on = KS == 3 && STRIDE == 1 && !UP && !RIDER && PREC == CONVH_STAMP_PREC && lane == 0 && (wave == 0 || wave == 7) &&
                        blockIdx.x < 256 && Cin == CONVH_STAMP_CIN && p.Cout == CONVH_STAMP_COUT;
#endif
  H_STAMP();   // 0: start

  // ---- staging indices (chunk invariant): thread -> (halo pixel row0 + i*128, float4 slot q) ----
  const int q = tid % Q4, row0 = tid / Q4;
  int in_pix[NIN];
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    const int pix = row0 + i * RPP;
    int v = -2;
    if (pix < NPIX) {
      const int hy = pix / HWD, hx = pix % HWD;
      const int iy = oy0 * STRIDE - PAD + hy, ix = ox0 * STRIDE - PAD + hx;
      if (UP) {
        const bool ok = iy >= 0 && iy < p.Hout && ix >= 0 && ix < p.Wout;
        v = ok ? (n * p.Hin + (iy >> 1)) * p.Win + (ix >> 1) : -1;
      } else {
        const bool ok = iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
        v = ok ? (n * p.Hin + iy) * p.Win + ix : -1;
      }
    }
    in_pix[i] = v;
  }

  using IO = ActIO<PREC>;
  typedef typename IO::Quad Quad;
  Quad rin[NIN];
  Quad rin2[RIDER ? NIN : 1];   // second prefetch set: the short rider chunks fetch two chunks ahead
  f32x4 rsc = {1.f, 1.f, 1.f, 1.f}, rsh = {0.f, 0.f, 0.f, 0.f};
  float satm = 0.f;   // f16x3 range guard: max |v| over the raw quads this thread staged (fdsr_act_io.h)
  const int nk = p.Cin_pad / KC;               // main chunks; chunks nk .. nk + nkr - 1 are the rider's (raw second input, centre tap)
  auto prefetch_to = [&](int kc, Quad* rin) {
    const ChunkSrc src = chunk_src<RIDER>(p, kc, KC, nk, q, gn);
    if (src.gn) {   // per-(image, channel) GroupNorm scale/shift travel with the input prefetch
      rsc = *reinterpret_cast<const f32x4*>(p.gn_scale + (size_t)n * Cin + src.cbase + q * 4);
      rsh = *reinterpret_cast<const f32x4*>(p.gn_shift + (size_t)n * Cin + src.cbase + q * 4);
    }
#pragma unroll
    for (int i = 0; i < NIN; ++i)   // branch-free: padding / unused rows read pixel 0 and are zeroed in stage()
      rin[i] = IO::load4(src.base, (size_t)(in_pix[i] < 0 ? 0 : in_pix[i]) * src.Cs + src.cc);
  };
  auto prefetch = [&](int kc) { prefetch_to(kc, rin); };
  auto stage_from = [&](int kc, unsigned char* buf, const Quad* rin) {
    const f32x4 sc = rsc, sh = rsh;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      if (NIN * RPP > NPIX && i == NIN - 1 && row0 + i * RPP >= NPIX) continue;   // only the last pass can overrun
      f32x4 v = IO::widen(rin[i]);
      if (gn && !(RIDER && kc >= nk)) {
        v = gn_act4(v, sc, sh, p.gn_plain);
      } else if (PREC == PREC_F16X3) {
        satm = sat_fold(satm, v);                      // a raw input the split below would clamp: tell the host (behind the K loops)
      }
      const float keep = in_pix[i] >= 0 ? 1.f : 0.f;   // conv zero-pads the ACTIVATED tensor
      const float lim = in_pix[i] >= 0 ? 65504.f : 0.f;   // f16 range clamp and zero padding in one med3
      unsigned char* dst = buf + (row0 + i * RPP) * ROWB + (q >> 2) * (NP * 32) + (q & 3) * 8;
      if (PREC == PREC_F16X3) {
        h4 hi, lo;
        split4_2step(v, lim, hi, lo);   // padding: lim = 0
        *reinterpret_cast<h4*>(dst) = hi;
        *reinterpret_cast<h4*>(dst + 32) = lo;
      } else {
        v = v * keep;
        *reinterpret_cast<uint2*>(dst) = stage4_16<PREC>(v);
      }
    }
  };
  auto stage = [&](int kc, unsigned char* buf) { stage_from(kc, buf, rin); };

  // ---- weight fragments: [cot][kc][wn][tap][plane][lane] x 16 B, loaded straight to VGPRs ----
  const uint4* wq = reinterpret_cast<const uint4*>(p.wq);
  const int nkt = RIDER ? nk + p.nkr : nk;
  uint4 Bf[T][NP];
  auto load_b_tap = [&](int kc, int tap) {
    const int ts = tap / KSUB, sub = tap % KSUB;   // packed per 16-channel block: [cot][kc16][wn][spatial tap]
    const uint4* src = wq + ((((size_t)cot * (nk * KSUB) + kc * KSUB + sub) * WN + wn) * (KS * KS) + ts) * (Cfg::WNP * 64) + lane;
    if (RIDER && kc >= nk)   // the 1x1 conv's own fragments [cot][kc16][wn]: one tap, into slot 0
      src = reinterpret_cast<const uint4*>(p.wq_r) + (((size_t)cot * p.nkr + (kc - nk)) * WN + wn) * (Cfg::WNP * 64) + lane;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) Bf[tap][pl] = src[pl * 64];
  };

  // ---- A fragment addresses: lane -> pixel column l&31 of a 32-pixel row, k half l>>5 ----
  const int r31 = lane & 31, h = lane >> 5;
  int abase[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int br = wm + mb * WM;   // tile row owned by this wave
    abase[mb] = ((br * STRIDE) * HWD + r31 * STRIDE) * ROWB + 16 * h;
  }

  f32x16 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;

  const int kc0 = ksi * nkt / SK, kc1 = (ksi + 1) * nkt / SK;   // this slice's chunks
#pragma unroll
  for (int tap = 0; tap < T; ++tap)
    if (tap == 0 || !(RIDER && kc0 >= nk)) load_b_tap(kc0, tap);
  prefetch(kc0);
  H_STAMP();   // 1: weight and input loads issued
  stage(kc0, sBuf0);
  H_STAMP();   // 2: first chunk staged (its loads have landed)
  if (kc0 + 1 < kc1) prefetch(kc0 + 1);
  __syncthreads();
  H_STAMP();   // 3: prologue barrier

  // A fragments are double-buffered over taps: the reads of tap t+1 are issued before the MFMAs
  // of tap t, so LDS latency hides under 3*MB MFMAs instead of being exposed per read.
  uint4 Af[2][MB][NP];
  const unsigned char* arow[MB];   // per chunk: halo buffer + this lane's row base; taps are immediates
  auto load_a = [&](int slot, int tap) {
    const int ts = tap / KSUB, sub = tap % KSUB;
    const int ky = ts / KS, kx = ts % KS;
    const int aoff = (ky * HWD + kx) * ROWB + sub * (NP * 32);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int pl = 0; pl < NP; ++pl)
        Af[slot][mb][pl] = *reinterpret_cast<const uint4*>(arow[mb] + aoff + 32 * pl);
  };

  // main chunks: all taps of 16 GroupNorm'ed channels
  const int kcm = RIDER ? (kc1 < nk ? kc1 : nk) : kc1;
  for (int kc = kc0; kc < kcm; ++kc) {
    unsigned char* cur = ((kc - kc0) & 1) ? sBuf1 : sBuf0;
    unsigned char* nxt = ((kc - kc0) & 1) ? sBuf0 : sBuf1;
    const bool more = kc + 1 < kc1;
    const bool next_rider = RIDER && kc + 1 >= nk;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) arow[mb] = cur + abase[mb];
    load_a(0, 0);
#pragma unroll
    for (int tap = 0; tap < T; ++tap) {
      if (tap + 1 < T) load_a((tap + 1) & 1, tap + 1);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const uint4 ahi = Af[tap & 1][mb][0];
        if (PREC == PREC_F16X3) {
          const uint4 alo = Af[tap & 1][mb][NP - 1];
          acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, alo), __builtin_bit_cast(h8, Bf[tap][0]), acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, ahi), __builtin_bit_cast(h8, Bf[tap][NP - 1]), acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, ahi), __builtin_bit_cast(h8, Bf[tap][0]), acc[mb], 0, 0, 0);
        } else {
          acc[mb] = mfma32_k16<PREC>(ahi, Bf[tap][0], acc[mb]);
        }
      }
      if (more && (tap == 0 || !next_rider)) load_b_tap(kc + 1, tap);   // same registers, next chunk
      if (tap == T / 2 && more) {                    // mid-chunk: fill the other halo buffer
        H_STAMP();   // per chunk +0: taps 0..T/2 issued
#ifdef CONVH_KO_STAGE   // perf-only bound (wrong results): no in-loop staging for this precision
        if (PREC != CONVH_KO_STAGE) {
          stage(kc + 1, nxt);
          if (kc + 2 < kc1) prefetch(kc + 2);
        }
#else
        stage(kc + 1, nxt);
        if (kc + 2 < kc1) prefetch(kc + 2);
#endif
        H_STAMP();   // +1: next chunk staged
      }
    }
    H_STAMP();       // +2: all taps issued
    __syncthreads();
    H_STAMP();       // +3: chunk barrier
  }
  if (RIDER && kc1 > nk) {
    // rider chunks: 16 raw channels of the second input each, centre tap only, the 1x1 conv's fragments in slot 0
    if (kc0 < nk) {   // the accumulators leave the main conv's weight scale for the rider's (a power of two: exact)
      const float ratio = (p.w_inv_scale_dev ? *p.w_inv_scale_dev : p.w_inv_scale) / (p.w_inv_scale_r_dev ? *p.w_inv_scale_r_dev : p.w_inv_scale_r);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) acc[mb] *= ratio;
    }
    // A rider chunk is short (MB x 3 MFMAs): its input is fetched TWO chunks ahead, into two register sets that alternate
    // (on entry `rin` holds chunk k0 + 1, as the main loop leaves it; the weight registers of taps 1..8 are free by now).
    const int k0 = kc0 > nk ? kc0 : nk;
    if (k0 + 2 < kc1) prefetch_to(k0 + 2, rin2);
    auto rider_chunk = [&](int kc, Quad* r1, Quad* r2) {   // r1 holds chunk kc + 1, r2 chunk kc + 2
      unsigned char* cur = ((kc - kc0) & 1) ? sBuf1 : sBuf0;
      unsigned char* nxt = ((kc - kc0) & 1) ? sBuf0 : sBuf1;
      (void)r2;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) arow[mb] = cur + abase[mb];
      load_a(0, T / 2);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const uint4 ahi = Af[0][mb][0];
        if (PREC == PREC_F16X3) {
          const uint4 alo = Af[0][mb][NP - 1];
          acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, alo), __builtin_bit_cast(h8, Bf[0][0]), acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, ahi), __builtin_bit_cast(h8, Bf[0][NP - 1]), acc[mb], 0, 0, 0);
          acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, ahi), __builtin_bit_cast(h8, Bf[0][0]), acc[mb], 0, 0, 0);
        } else {
          acc[mb] = mfma32_k16<PREC>(ahi, Bf[0][0], acc[mb]);
        }
      }
      if (kc + 1 < kc1) {
        load_b_tap(kc + 1, 0);
        stage_from(kc + 1, nxt, r1);
        if (kc + 3 < kc1) prefetch_to(kc + 3, r1);
      }
      __syncthreads();
    };
    for (int kc = k0; kc < kc1; kc += 2) {
      rider_chunk(kc, rin, rin2);
      if (kc + 1 < kc1) rider_chunk(kc + 1, rin2, rin);
    }
  }
  if (PREC == PREC_F16X3) sat_raise(p.sat_flag, satm, 65504.f);   // the range guard's one store, behind the last K chunk

  // ---- epilogue.  Interior tiles take a branch-free path: per-element bounds branches make the
  // compiler wait vmcnt(0) before every store.  Each lane also sums its outputs per channel
  // (sum, sumsq): the consumer's GroupNorm statistics, reduced in a fixed order. ----
  const int co = co0 + wn * 32 + r31;
  const bool cok = co < p.Cout;
  // unconditional loads (clamped channel, noise shift through a 0 / 1 factor): one round trip, not three
  const float* tembp = p.temb ? p.temb + (size_t)n * p.temb_stride + p.temb_off : p.bias;
  const float add = epi_add1<RIDER>(p.bias, p.bias_r, tembp, p.temb ? 1.f : 0.f, cok ? co : 0);
  float s1 = 0.f, s2 = 0.f;
  const float winv_m = p.w_inv_scale_dev ? *p.w_inv_scale_dev : p.w_inv_scale;   // uniform: a scalar load
  const float winv = RIDER ? (p.w_inv_scale_r_dev ? *p.w_inv_scale_r_dev : p.w_inv_scale_r) : winv_m;
  if (RIDER && kc1 <= nk) {   // (split K) a slice that never reached the rider chunks: bring it to the rider's scale too
    const float ratio = winv_m / winv;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[mb] *= ratio;
  }
  const bool interior = (oy0 + TH <= p.Hout) && (ox0 + TW <= p.Wout) && (co0 + BN <= p.Cout);
  if (SK > 1) {   // raw partial accumulators; bias, shift, residual and statistics happen in the reduce
    float* sb = p.kscratch + (size_t)ksi * p.N * p.Hout * p.Wout * p.Cout;
    if (interior) {
      float* obase = sb + ((size_t)(n * p.Hout + oy0 + wm) * p.Wout + ox0 + 4 * h) * p.Cout + co;
      const size_t rstride = (size_t)WM * p.Wout * p.Cout;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) obase[mb * rstride + (size_t)((i & 3) + 8 * (i >> 2)) * p.Cout] = acc[mb][i];
    } else {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int oy = oy0 + wm + mb * WM, ox = ox0 + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (cok && oy < p.Hout && ox < p.Wout) sb[((size_t)(n * p.Hout + oy) * p.Wout + ox) * p.Cout + co] = acc[mb][i];
        }
    }
    return;
  }
  // OUT16: this launch stores bf16 (bf16 mode, every conv but the last); residuals follow the activation type
  auto epilogue = [&](auto out16_tag) {
    constexpr bool OUT16 = decltype(out16_tag)::value;
    auto put = [&](size_t idx, float v) {
      if (OUT16) reinterpret_cast<unsigned short*>(p.out)[idx] = PREC == PREC_F16 ? f32_to_f16_bits(v) : f32_to_bf16_bits(v);
      else p.out[idx] = v;
    };
    if (interior) {
      const size_t obase = ((size_t)(n * p.Hout + oy0 + wm) * p.Wout + ox0 + 4 * h) * p.Cout + co;
      const size_t rstride = (size_t)WM * p.Wout * p.Cout;
      float rv[MB][16];
      if (p.res) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int i = 0; i < 16; ++i) rv[mb][i] = IO::load1(p.res, obase + mb * rstride + (size_t)((i & 3) + 8 * (i >> 2)) * p.Cout);
      } else {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int i = 0; i < 16; ++i) rv[mb][i] = 0.f;
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc[mb][i] * winv + add + rv[mb][i];
          put(obase + mb * rstride + (size_t)((i & 3) + 8 * (i >> 2)) * p.Cout, v);
          s1 += v;
          s2 += v * v;
        }
    } else {
      float rv[MB][16];
      if (p.res) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int oy = oy0 + wm + mb * WM, ox = ox0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool ok = cok && oy < p.Hout && ox < p.Wout;
            rv[mb][i] = ok ? IO::load1(p.res, ((size_t)(n * p.Hout + oy) * p.Wout + ox) * p.Cout + co) : 0.f;
          }
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int oy = oy0 + wm + mb * WM, ox = ox0 + (i & 3) + 8 * (i >> 2) + 4 * h;
          if (cok && oy < p.Hout && ox < p.Wout) {
            float v = acc[mb][i] * winv + add;
            if (p.res) v += rv[mb][i];
            put(((size_t)(n * p.Hout + oy) * p.Wout + ox) * p.Cout + co, v);
            s1 += v;
            s2 += v * v;
          }
        }
    }
  };
  H_STAMP();   // epilogue starts (accumulators final)
  if (prec_is16(PREC) && !p.out_f32) epilogue(std::true_type{});
  else epilogue(std::false_type{});
  H_STAMP();   // stores issued
  if (p.part_out) {
    // the main loop ended with a barrier: the halo buffers are free
    float* sp = reinterpret_cast<float*>(smem_h);   // [WM][BN][2]
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (h == 0) {
      sp[(wm * BN + wn * 32 + r31) * 2 + 0] = s1;
      sp[(wm * BN + wn * 32 + r31) * 2 + 1] = s2;
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
  H_STAMP();   // end
}

#ifdef CONVH_STAMPS
extern "C" int fdsr_diag_convh_stamps(unsigned long long* dst, size_t count) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_h_stamps), count * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif

// Split-K second phase: sums the ksplit partial outputs in slice order, applies bias + noise-embedding
// shift + residual, stores NHWC and emits the per-tile channel statistics.  One workgroup per
// 2 x 32 output pixels (the smallest conv tile, so the partials fit the same appendix) x cb channels.
// The kernel is nothing but latency (37 of these launches per B = 1 forward): EVERY load is unconditional -- optional operands read a
// valid stand-in address and are dropped by a select, out-of-range pixels read a clamped one -- and issued before the first use of any
// of them: bias, rider bias, noise shift, un-scaling factor, the NS slices of a pixel quad and its residual are ONE memory round trip.
// (With `if (p.temb)` / `if (p.res)` / `if (s < ksplit)` around the loads the compiler put an s_waitcnt vmcnt(0) behind each branch:
// five serial round trips, 7.2 us per launch.)  NS = the K split rounded up to a power of two (slices past ksplit re-read the last one
// and are dropped); OUT16: bf16 activations.
// CB32: cb == 32 (every Cout that is a multiple of 32): a thread owns one channel quad of the two pixels (row 0 and row 1, column g) of the tile, and
// the loads of both are in flight before anything is used.
template <int NS, bool OUT16, bool CB32>
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const ConvParams p, const int cb) {
  __shared__ float sred[256 * 8];
  const int tilesX = (p.Wout + 31) / 32;
  const int tile = blockIdx.x, n = blockIdx.y;
  const int tx = tile % tilesX, ty = tile / tilesX;
  const int cq = CB32 ? 8 : cb >> 2, groups = CB32 ? 32 : 256 / cq, cbase = blockIdx.z * cb;
  const int tid = threadIdx.x, c4 = tid % cq, g = tid / cq;
  const int cch = cbase + c4 * 4;
  const bool has_r = p.xr0 != nullptr, has_t = p.temb != nullptr, has_res = p.res != nullptr;
  // per-channel constants and the un-scaling factor.  Stand-ins are addresses nothing else loads from (the compiler would otherwise
  // reuse the loaded value and put the real load back under a branch).
  const f32x4 bias = *reinterpret_cast<const f32x4*>(p.bias + cch);
  const f32x4 bias_r = *reinterpret_cast<const f32x4*>(has_r ? p.bias_r + cch : p.bias + cbase);
  const f32x4 temb = *reinterpret_cast<const f32x4*>(has_t ? p.temb + (size_t)n * p.temb_stride + p.temb_off + cch : p.bias + cbase);
  const float* wdev = has_r ? p.w_inv_scale_r_dev : p.w_inv_scale_dev;
  const float wload = *(wdev ? wdev : p.bias);
  const size_t slice = (size_t)p.N * p.Hout * p.Wout * p.Cout;
  const int last = p.ksplit - 1;
  const float* resp = has_res ? p.res : p.out;   // (no residual: this launch's own output location, read and dropped)
  constexpr int NPX = CB32 ? 2 : 1;
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  auto pixels = [&](int px0) __attribute__((always_inline)) {
    f32x4 sl[NPX][NS], rv[NPX];
    size_t o[NPX];
    bool ok[NPX];
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
      const int px = px0 + i * groups;
      const int oy = ty * 2 + (px >> 5), ox = tx * 32 + (px & 31);
      ok[i] = g < groups && px < 64 && oy < p.Hout && ox < p.Wout;
      o[i] = ((size_t)(n * p.Hout + min(oy, p.Hout - 1)) * p.Wout + min(ox, p.Wout - 1)) * p.Cout + cch;
#pragma unroll
      for (int s = 0; s < NS; ++s) sl[i][s] = *reinterpret_cast<const f32x4*>(p.kscratch + (size_t)min(s, last) * slice + o[i]);
      if (OUT16) rv[i] = p.out_bf16 == 2 ? ActIO<PREC_F16>::widen(ActIO<PREC_F16>::load4(resp, o[i])) : ActIO<PREC_BF16>::widen(ActIO<PREC_BF16>::load4(resp, o[i]));
      else rv[i] = *reinterpret_cast<const f32x4*>(resp + o[i]);
    }
    __builtin_amdgcn_sched_barrier(0);   // every load above is issued before the first wait below (the scheduler otherwise waits for the constants first)
    const float winv = wdev ? wload : (has_r ? p.w_inv_scale_r : p.w_inv_scale);
    f32x4 add = bias;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      add[e] += has_r ? bias_r[e] : 0.f;
      add[e] += has_t ? temb[e] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
      f32x4 a = sl[i][0];
#pragma unroll
      for (int s = 1; s < NS; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] += s <= last ? sl[i][s][e] : 0.f;
      a = a * winv + add;
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += has_res ? rv[i][e] : 0.f;
      // (the sums take the value through a select, not under the branch of the store: with every use under `if (ok)` the compiler
      // sinks the pixel's loads into that branch, behind the wait of the pixel before it)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = ok[i] ? a[e] : 0.f;
        s1[e] += v;
        s2[e] += v * v;
      }
      if (ok[i]) {
        if (OUT16) {
          *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p.out) + o[i]) = p.out_bf16 == 2 ? pack4_16<PREC_F16>(a) : pack4_16<PREC_BF16>(a);
        } else {
          *reinterpret_cast<f32x4*>(p.out + o[i]) = a;
        }
      }
    }
  };
  if (CB32) pixels(g);   // one straight-line pass: the constants' loads and the 2 (NS + 1) pixel loads are issued together
  else for (int px0 = g; px0 < 64; px0 += groups) pixels(px0);
  if (p.part_out) {
    if (g < groups) {
      *reinterpret_cast<f32x4*>(sred + (g * cq + c4) * 8) = s1;
      *reinterpret_cast<f32x4*>(sred + (g * cq + c4) * 8 + 4) = s2;
    }
    __syncthreads();
    if (tid < cq) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
      for (int gg = 0; gg < groups; ++gg) {
        a += *reinterpret_cast<const f32x4*>(sred + (gg * cq + tid) * 8);
        b += *reinterpret_cast<const f32x4*>(sred + (gg * cq + tid) * 8 + 4);
      }
      float* dst = p.part_out + (((size_t)n * gridDim.x + tile) * p.Cout + cbase + tid * 4) * 2;
#pragma unroll
      for (int e = 0; e < 4; ++e) { dst[2 * e] = a[e]; dst[2 * e + 1] = b[e]; }
      if (p.gsum_out) {   // the consumer-side GroupNorm (ConvParams::gsum_out): this tile's sums of the thread's two channel pairs
        const int pair = (cbase + tid * 4) >> 1;
        const int xcd = xcc_id();
        gsum_add(p.gsum_out, n, p.Cout >> 1, pair, xcd, a[0] + a[1], b[0] + b[1]);
        gsum_add(p.gsum_out, n, p.Cout >> 1, pair + 1, xcd, a[2] + a[3], b[2] + b[3]);
      }
    }
  }
}

static hipError_t launch_splitk_reduce(const ConvParams& q, int rt, int cb, hipStream_t s) {
  const dim3 grid(rt, q.N, q.Cout / cb), block(256);
#define SKR(NS_)                                                                                                   \
  if (q.ksplit <= NS_) {                                                                                           \
    if (cb == 32) {                                                                                                \
      if (q.out_bf16) hipLaunchKernelGGL((splitk_reduce_kernel<NS_, true, true>), grid, block, 0, s, q, cb);       \
      else hipLaunchKernelGGL((splitk_reduce_kernel<NS_, false, true>), grid, block, 0, s, q, cb);                 \
    } else {                                                                                                       \
      if (q.out_bf16) hipLaunchKernelGGL((splitk_reduce_kernel<NS_, true, false>), grid, block, 0, s, q, cb);      \
      else hipLaunchKernelGGL((splitk_reduce_kernel<NS_, false, false>), grid, block, 0, s, q, cb);                \
    }                                                                                                              \
    return hipGetLastError();                                                                                      \
  }
  SKR(2) SKR(4) SKR(8) SKR(16)
#undef SKR
  return hipErrorInvalidValue;
}

template <int KS, int STRIDE, bool UP, int TH, int WN, int PREC, int KSUB, bool RIDER = false>
static hipError_t launch_h_t(const ConvParams& p, hipStream_t s, int* tiles) {
  using Cfg = ConvHCfg<KS, STRIDE, UP, TH, WN, PREC, KSUB>;
  auto kfn = conv_mfma_h_kernel<KS, STRIDE, UP, TH, WN, PREC, KSUB, RIDER>;
  const size_t lds = (size_t)2 * Cfg::BUF_BYTES;
  const int tilesX = (p.Wout + Cfg::TW - 1) / Cfg::TW, tilesY = (p.Hout + TH - 1) / TH;
  if (tiles) *tiles = tilesX * tilesY;
  const int sk = p.ksplit > 1 ? p.ksplit : 1;
  const int nwg = p.N * tilesX * tilesY * (p.Cout_pad / Cfg::BN) * sk;
  ConvParams q = p;
  q.out_bf16 = p.out_f32 ? 0 : prec_act16(PREC);
  if (KS == 3 && STRIDE == 1 && !UP && KSUB == 1 && (PREC == PREC_F16X3 || prec_is16(PREC)) && conv_k32_ok(TH, WN, PREC, q)) {
    const hipError_t e = launch_conv_k32(TH, WN, PREC, q, nwg, s);   // the 16x16x32 form (fdsr_conv_k32.hip): same grid, same outputs
    if (e != hipSuccess) return e;
  } else {
    if (p.gb_x0 || p.drop_mask || p.gs0) return hipErrorInvalidValue;   // the GroupNorm-backward epilogue, the dropout staging and the consumer-side GroupNorm live in the 16x16x32 kernels only (conv_h_gnb_ok / conv_h_drop_ok / conv_h_gnc_ok)
    hipLaunchKernelGGL(kfn, dim3(nwg), dim3(Cfg::NT), lds, s, q);
  }
  if (sk > 1 && (g_tun.knockout & 2)) {   // timing-only probe: the reduce launch left out (results are garbage)
    if (tiles) *tiles = ((p.Wout + 31) / 32) * ((p.Hout + 1) / 2);
  } else if (sk > 1) {
    const int rt = ((p.Wout + 31) / 32) * ((p.Hout + 1) / 2);
    if (tiles) *tiles = rt;
    const int cb = p.Cout % 32 == 0 ? 32 : p.Cout;
    const hipError_t e = launch_splitk_reduce(q, rt, cb, s);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

template <int KS, int STRIDE, bool UP, int TH, int WN, int PREC, int KSUB, bool RIDER = false>
static hipError_t init_h_t() {
  auto kfn = conv_mfma_h_kernel<KS, STRIDE, UP, TH, WN, PREC, KSUB, RIDER>;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// X(KS, STRIDE, UP, TH, WN, KSUB): TH rows of 32 pixels, WN of the 8 waves along Cout;
// TH % (8/WN) == 0 and at most 4 accumulator tiles (64 VGPRs) per wave.
#define FDSR_CONVH_SHAPES(X)                                                                                   \
  X(3, 1, false, 8, 4, 1) X(3, 1, false, 4, 4, 1) X(3, 1, false, 16, 2, 1) X(3, 1, false, 8, 2, 1) X(3, 1, false, 4, 2, 1) \
  X(3, 1, false, 16, 1, 1) X(3, 1, false, 8, 1, 1) X(3, 1, false, 4, 8, 1) X(3, 1, false, 2, 8, 1)                       \
  X(3, 1, true, 4, 8, 1) X(3, 1, true, 2, 8, 1) X(3, 2, false, 4, 8, 1)                                                  \
  X(3, 1, true, 8, 4, 1) X(3, 1, true, 4, 4, 1) X(3, 1, true, 16, 2, 1) X(3, 1, true, 8, 2, 1) X(3, 1, true, 4, 2, 1)      \
  X(3, 2, false, 4, 4, 1) X(3, 2, false, 4, 2, 1)                                                                        \
  X(1, 1, false, 8, 4, 1) X(1, 1, false, 4, 4, 1) X(1, 1, false, 16, 2, 1) X(1, 1, false, 8, 2, 1) X(1, 1, false, 4, 2, 1) \
  X(1, 1, false, 16, 1, 1) X(1, 1, false, 8, 1, 1) X(1, 1, false, 4, 8, 1) X(1, 1, false, 2, 8, 1)                       \
  X(1, 1, false, 8, 4, 4) X(1, 1, false, 4, 4, 4) X(1, 1, false, 8, 2, 4) X(1, 1, false, 4, 2, 4)                         \
  X(1, 1, false, 8, 1, 4) X(1, 1, false, 4, 8, 4) X(1, 1, false, 2, 8, 4)

// the stride-1 3x3 shapes, again with a 1x1 rider: XR(TH, WN)
#define FDSR_CONVH_RIDER_SHAPES(XR) \
  XR(8, 4) XR(4, 4) XR(16, 2) XR(8, 2) XR(4, 2) XR(16, 1) XR(8, 1) XR(4, 8) XR(2, 8)

// Output-channel split of the workgroup (weights are packed per WN, so this depends on the layer only).
void conv_h_config(ConvKind kind, int Cout, int* TH, int* WN) {
  *WN = Cout >= 256 ? 8 : (Cout >= 128 ? 4 : (Cout >= 64 ? 2 : 1));   // 256-wide tiles: the input is staged once
  if ((kind == CONV3_S2 || kind == CONV3_UP) && *WN == 1) *WN = 2;
  *TH = kind == CONV3_S2 ? 4 : 8;   // default; launch_conv_h picks the final TH from the grid size
}

// Rows per workgroup tile, chosen per launch: the largest tile (<= 4 accumulator tiles per wave) that
// still gives every CU a workgroup (measured: a threshold of 256 workgroups beats 512 by 3-4 % at batch
// 1-4 and is neutral at 16-64; 128 loses); smaller feature maps fall back to the smallest tile and split K.
static int pick_th(ConvKind kind, int WN, int ksub, const ConvParams& p) {
  if (kind == CONV3_S2) return 4;
  const int WM = 8 / WN;
  const int tilesX = (p.Wout + 31) / 32, nco = p.Cout_pad / (32 * WN);
  int best = -1;
  for (int th = 16; th >= 2; th >>= 1) {
    if (th % WM || th / WM > 4) continue;
    if (th < 4 && WN < 8) continue;
    if (ksub > 1 && th > 8) continue;          // LDS: 64-channel rows
    const long wgs = (long)p.N * tilesX * ((p.Hout + th - 1) / th) * nco;
    best = th;
    if (wgs >= g_tun.th_min_wgs) break;   // default 256: one workgroup per CU
  }
  return best;
}

int conv_h_ksplit(ConvKind kind, int N, int Hout, int Wout, int Cout, int Cout_pad, int Cin_pad, int C0, int C1) {
  if (!g_tun.splitk || kind == CONV3_UP || (Cout & 3) || Cout > 1024) return 1;
  int TH, WN;
  conv_h_config(kind, Cout, &TH, &WN);
  const int ksub = (kind == CONV1 && Cin_pad % 64 == 0 && (C1 == 0 || C0 % 64 == 0)) ? 4 : 1;
  ConvParams p{};
  p.N = N; p.Hout = Hout; p.Wout = Wout; p.Cout_pad = Cout_pad;
  TH = pick_th(kind, WN, ksub, p);
  const long wgs = (long)N * ((Wout + 31) / 32) * ((Hout + TH - 1) / TH) * (Cout_pad / (32 * WN));
  const int nk = Cin_pad / (16 * ksub);
  const int target = g_tun.sk_target;
  if (wgs >= target) return 1;
  // enough slices to give every CU a workgroup, at least two chunks per slice
  const int sk = (int)std::min<long>(std::min(16, nk / 2), (target + wgs - 1) / wgs);
  return sk >= 2 ? sk : 1;
}

// would launch_conv_h run this launch on a kernel that has the GroupNorm-backward epilogue (ConvParams::gb_*)?  The training step asks
// before it sets the gb_* fields; a launch that carries them and lands elsewhere fails.
bool conv_h_gnb_ok(ConvKind kind, int prec, const ConvParams& p) {
  if (kind != CONV3_S1 || prec != PREC_F16X3 || p.xr0 || p.res || p.ksplit > 1 || !p.out_f32 || p.gn_scale) return false;
  int TH, WN;
  conv_h_config(kind, p.Cout, &TH, &WN);
  if (WN == 2 && conv_k32_small_ok(kind, prec, p)) return true;
  TH = pick_th(kind, WN, 1, p);
  return conv_k32_ok(TH, WN, prec, p);
}

// the same question for train-mode dropout applied in the staging (ConvParams::drop_mask in a 16-bit launch)
bool conv_h_drop_ok(ConvKind kind, int prec, const ConvParams& p) {
  if (kind != CONV3_S1 || !conv_k32_drop_ok(prec, p)) return false;
  int TH, WN;
  conv_h_config(kind, p.Cout, &TH, &WN);
  if (WN == 2 && conv_k32_small_ok(kind, prec, p)) return true;
  TH = pick_th(kind, WN, 1, p);
  return conv_k32_ok(TH, WN, prec, p);
}

// the consumer-side GroupNorm (ConvParams::gs0): would this launch land on a GNC instantiation?  (the launch's dispatch, replayed)
bool conv_h_gnc_ok(ConvKind kind, int prec, const ConvParams& p) {
  if (!g_tun.gn_consumer || kind != CONV3_S1 || prec == PREC_F32) return false;
  int TH, WN;
  conv_h_config(kind, p.Cout, &TH, &WN);
  ConvParams q = p;                       // as the other forms see a GroupNorm'd launch
  q.gn_scale = q.gn_shift = reinterpret_cast<const float*>(p.gs_gamma);
  if ((WN == 2 || WN == 4) && conv_strip_ok(kind, prec, q)) return false;
  if (WN == 2 && conv_k32_small_ok(kind, prec, q)) return false;
  TH = pick_th(kind, WN, 1, p);
  return conv_k32_gnc_ok(TH, WN, prec, p);
}

// does this launch's kernel add its output's channel-pair sums to ConvParams::gsum_out?  A K split ends in splitk_reduce (32-channel
// blocks); without one: the 16x16x32 kernels (tile and small-workgroup forms, and the sub-pixel upsample form)
bool conv_h_gsum_ok(ConvKind kind, int prec, const ConvParams& p, bool sub_pixel_up2) {
  if (!g_tun.gn_consumer || prec == PREC_F32 || (p.Cout & 3)) return false;
  if (p.ksplit > 1) return p.Cout % 32 == 0 && !(g_tun.knockout & 2);
  if (kind == CONV3_UP) return sub_pixel_up2 && conv_up2_k32_ok(prec, p);
  if (kind != CONV3_S1) return false;
  int TH, WN;
  conv_h_config(kind, p.Cout, &TH, &WN);
  if ((WN == 2 || WN == 4) && conv_strip_ok(kind, prec, p)) return false;
  if (WN == 2 && conv_k32_small_ok(kind, prec, p)) return true;
  TH = pick_th(kind, WN, 1, p);
  return conv_k32_ok(TH, WN, prec, p);
}

hipError_t launch_conv_h(ConvKind kind, int prec, const ConvParams& p, hipStream_t s, int* tiles) {
  int TH, WN;
  conv_h_config(kind, p.Cout, &TH, &WN);
  // 1x1: stage 64 input channels per barrier when the (concatenated) input allows it
  const int ksub = (kind == CONV1 && p.Cin_pad % 64 == 0 && (p.C1 == 0 || p.C0 % 64 == 0)) ? 4 : 1;
  // 64-cout launches of large grids: the small-workgroup form of the 16x16x32 kernel (two workgroups per CU) with tile rows of its own
  if ((WN == 2 || WN == 4) && ksub == 1 && conv_strip_ok(kind, prec, p)) return launch_conv_strip(prec, p, WN, s, tiles);   // (64- and 128-cout launches)
  if (WN == 2 && ksub == 1 && conv_k32_small_ok(kind, prec, p)) return launch_conv_k32_small(prec, p, s, tiles);
  TH = pick_th(kind, WN, ksub, p);
  const int ks = kind == CONV1 ? 1 : 3, stride = kind == CONV3_S2 ? 2 : 1;
  const bool up = kind == CONV3_UP;
  if (p.xr0) {   // 3x3 stride-1 with a 1x1 rider
    if (kind != CONV3_S1) return hipErrorInvalidValue;
#define XR(TH_, WN_)                                                                                     \
    if (TH == TH_ && WN == WN_)                                                                          \
      return prec == PREC_F16X3 ? launch_h_t<3, 1, false, TH_, WN_, PREC_F16X3, 1, true>(p, s, tiles)     \
                                : prec == PREC_F16 ? launch_h_t<3, 1, false, TH_, WN_, PREC_F16, 1, true>(p, s, tiles) : launch_h_t<3, 1, false, TH_, WN_, PREC_BF16, 1, true>(p, s, tiles);
    FDSR_CONVH_RIDER_SHAPES(XR)
#undef XR
    return hipErrorInvalidValue;
  }
#define X(KS_, ST_, UP_, TH_, WN_, KSUB_)                                                                \
  if (ks == KS_ && stride == ST_ && up == UP_ && TH == TH_ && WN == WN_ && ksub == KSUB_) {               \
    return prec == PREC_F16X3 ? launch_h_t<KS_, ST_, UP_, TH_, WN_, PREC_F16X3, KSUB_>(p, s, tiles)       \
                              : prec == PREC_F16 ? launch_h_t<KS_, ST_, UP_, TH_, WN_, PREC_F16, KSUB_>(p, s, tiles) : launch_h_t<KS_, ST_, UP_, TH_, WN_, PREC_BF16, KSUB_>(p, s, tiles);       \
  }
  FDSR_CONVH_SHAPES(X)
#undef X
  return hipErrorInvalidValue;
}

hipError_t kernels_h_init() {
  hipError_t e;
#define X(KS_, ST_, UP_, TH_, WN_, KSUB_)                                                          \
  if ((e = init_h_t<KS_, ST_, UP_, TH_, WN_, PREC_F16X3, KSUB_>()) != hipSuccess) return e;         \
  if ((e = init_h_t<KS_, ST_, UP_, TH_, WN_, PREC_BF16, KSUB_>()) != hipSuccess) return e; \
  if ((e = init_h_t<KS_, ST_, UP_, TH_, WN_, PREC_F16, KSUB_>()) != hipSuccess) return e;
  FDSR_CONVH_SHAPES(X)
#undef X
#define XR(TH_, WN_)                                                                                    \
  if ((e = init_h_t<3, 1, false, TH_, WN_, PREC_F16X3, 1, true>()) != hipSuccess) return e;              \
  if ((e = init_h_t<3, 1, false, TH_, WN_, PREC_BF16, 1, true>()) != hipSuccess) return e; \
  if ((e = init_h_t<3, 1, false, TH_, WN_, PREC_F16, 1, true>()) != hipSuccess) return e;
  FDSR_CONVH_RIDER_SHAPES(XR)
#undef XR
  if ((e = kernels_k32_init()) != hipSuccess) return e;
  return kernels_strip_init();
}

}  // namespace fdsr
