// HAT (MSI_SR_model/model/hat.py: GeneratorResNet, upsampler='pixelshuffle', resi_connection='1conv', patch_size 1, ape=False)
// inference in exact fp32 on gfx950.
//
//   x    = (reflect_pad(img, to a multiple of 16) - mean) * img_range                      NCHW -> NHWC       swin_input_kernel
//   f    = conv_first(x);  t = patch_embed.norm(f)
//   per RHAG: depth HABs, one OCAB, t = conv(t) + t_in
//     HAB:   n = norm1(t);  t += proj(window_attention(qkv(n))) + conv_scale * gate * cab,   cab = conv(gelu(conv(n))),
//            gate = sigmoid(W2 relu(W1 mean_HW(cab) + b1) + b2);   t += fc2(gelu(fc1(norm2(t))))
//     OCAB:  n = norm1(t);  t += proj(attention(q of 16 x 16 windows, k / v of the 24 x 24 windows around them));  t += mlp(norm2(t))
//   y    = conv_after_body(norm(t)) + f;  y = leaky_relu(conv_before_upsample(y), 0.01)
//   y    = pixel_shuffle(conv(y)) per factor of two, ONE convolution for every stage (one conv + PixelShuffle(3) at scale 3);
//          out = conv_last(y) / img_range + mean at the PADDED size times the scale (the reference does not crop), NCHW
//
// The token GEMM, LayerNorm, the input kernel, the accumulator's row map and the attention kernel's chunk sizes (QB, KC, KP) are
// fdsr_swin_common.h's.  The walk of the network, its GEMM dispatcher, the
// common tensor kinds and the shape and configuration checks are fdsr_swin_walk.h's, shared with SwinIR; the host side here is
// HAT's block bodies (Walker::group: the HABs with their CAB branch, the OCAB), its kinds RPB_OCA and GATE, its one shared
// upsampling convolution, its traits and its extern "C" functions.  New here:
//   hat_attn_kernel<OCA>  one workgroup per (image, window, head, block of 32 queries).  The block's full score rows stay in
//                         LDS ([key][query], 256 or 576 keys): exact max / exp / sum / divide.  k, and after the softmax v, stream
//                         through LDS in chunks of 128 keys.  The roll, the partition, the region ids, the -100 mask, the bias
//                         (gathered and transposed at load) and the out-of-image test of an OCA key are addresses and LDS
//                         contents.  An OCA key outside the image is a zero k and a zero v: its logit is its bias alone and it
//                         counts in the denominator.
//   two GEMM epilogues    EPI_COLSUM stores the tile and leaves the column sums of each wave's 64 rows in a small buffer;
//                         EPI_HAB writes acc + bias + shortcut + conv_scale * gate[b][c] * cab[m][c].
//   hat_gate_kernel       per image: the partial sums in row order, / HW, the two 1x1 layers, ReLU, sigmoid.
// Every output element has one fixed summation order (no atomics, no split-K): reruns are bitwise equal and an image's result
// depends neither on B nor on its place in the batch.
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
#include "fdsr_swin_walk.h"

using namespace fdsr_int;

namespace {

constexpr int WS = 16, WT = WS * WS;       // the window and its tokens
constexpr int WSE = 24, WKT = WSE * WSE;   // the overlapping window (overlap_ratio 0.5) and its keys

enum HatEpi { EPI_COLSUM = EPI_EXT, EPI_HAB = EPI_EXT + 1 };

struct HatGemmArgs : GemmArgs {
  float* colsum;        // EPI_COLSUM: [M / 64][N]
  const float* gate;    // EPI_HAB: [B][N]
  const float* cab;     // EPI_HAB: [M][N]
  float conv_scale;
};

template <int EPI, class ARGS>
__device__ void gemm_epilogue_ext(const ARGS& p, const f32x16 (&acc)[2], int row0, int co, int h, float bias) {
  if constexpr (EPI == EPI_COLSUM) {
    // M is a multiple of 256 here (whole 16 x 16 windows): every row of the tile exists and 64 rows never span two images
    float s = 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int om = acc_row(row0 + mb * 32, i, h);
        const float v = acc[mb][i] + bias;
        p.out[(size_t)om * p.N + co] = v;
        s += v;
      }
    s += __shfl_xor(s, 32, 64);   // the other 32 rows of this column
    if (h == 0) p.colsum[(size_t)(row0 >> 6) * p.N + co] = s;
  } else {
    const int HW = p.H * p.W;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int om = acc_row(row0 + mb * 32, i, h);
        if (om >= p.M) continue;
        const size_t o = (size_t)om * p.N + co;
        const float v = acc[mb][i] + bias;
        // shortcut + attn_x + conv_x * conv_scale, conv_x = cab * gate
        p.out[o] = __fadd_rn(__fadd_rn(p.res[o], v), __fmul_rn(__fmul_rn(p.cab[o], p.gate[(size_t)(om / HW) * p.N + co]), p.conv_scale));
      }
  }
}

// ChannelAttention's gate of one image: mean over the map from the 64-row partial sums, in row order; Conv1x1 C -> Cs, ReLU,
// Conv1x1 Cs -> C, sigmoid.  w1 [Cs][C], w2 [C][Cs] as the checkpoint holds them.
__global__ void __launch_bounds__(256) hat_gate_kernel(const float* __restrict__ colsum, const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ gate,
                                                       int tiles, int C, int Cs, float hw) {
  __shared__ float sMean[LN_MAX_C], sHid[LN_MAX_C];
  const int b = blockIdx.x, t = threadIdx.x;
  for (int c = t; c < C; c += 256) {
    float s = 0.f;
    for (int k = 0; k < tiles; ++k) s += colsum[((size_t)b * tiles + k) * C + c];
    sMean[c] = s / hw;
  }
  __syncthreads();
  for (int r = t; r < Cs; r += 256) {
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += w1[(size_t)r * C + c] * sMean[c];
    sHid[r] = fmaxf(a + b1[r], 0.f);
  }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    float a = 0.f;
    for (int r = 0; r < Cs; ++r) a += w2[(size_t)c * Cs + r] * sHid[r];
    gate[(size_t)b * C + c] = 1.f / (1.f + expf(-(a + b2[c])));
  }
}

// the tap 'cab': the gated CAB output, which the forward never stores (proj's epilogue forms it)
__global__ void __launch_bounds__(256) hat_gate_mul_kernel(const float* __restrict__ cab, const float* __restrict__ gate, float* __restrict__ y,
                                                           int HW, int C, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t m = i / C;
  y[i] = __fmul_rn(cab[i], gate[(m / HW) * C + (i - m * C)]);
}

// Attention of one (image, window, head, block of QB queries).  qkv: [B][H W][3 C], a token's row is q | k | v, each head-major.
// Query token (ty, tx) of window (wy, wx) is the pixel ((wy 16 + ty + shift) mod H, (wx 16 + tx + shift) mod W) -- torch.roll
// by -shift, then window_partition -- and the output goes back to the same pixel.
//   OCA = false: the keys are the window's own 256 tokens; biasT [heads][256 keys][256 queries]; shift > 0: tokens of different
//                regions of the rolled image (three slices per axis: [0, H - 16), [H - 16, H - shift), [H - shift, H)) get -100.
//   OCA = true:  shift = 0; key (ky, kx), 0 <= ky, kx < 24, is the pixel (wy 16 - 4 + ky, wx 16 - 4 + kx) -- nn.Unfold(24, stride
//                16, padding 4) of the qkv output -- and a zero k and v outside the image; biasT [heads][576 keys][256 queries].
template <bool OCA>
__global__ void __launch_bounds__(256) hat_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ biasT, float* __restrict__ out,
                                                       int H, int W, int C, int heads, int hd, int shift, float scale) {
  constexpr int NK = OCA ? WKT : WT;
  __shared__ float sSt[NK * QB];    // [key][query]: the scores, then the probabilities
  __shared__ float sQt[HD * QB];    // [d][query], q * scale
  __shared__ float sKV[HD * KP];    // a chunk of k as [d][key] (pitch KP), then of v as [key][d]
  __shared__ float sRed[8 * QB];
  __shared__ int sKPix[NK];         // the pixel of a key, -1 outside the image
  __shared__ int sKRid[OCA ? 1 : NK];
  __shared__ int sQPix[QB], sQRid[QB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nwx = W / WS, nwin = nwx * (H / WS);
  int bx = blockIdx.x;
  const int qb = bx % (WT / QB);
  bx /= WT / QB;
  const int head = bx % heads;
  bx /= heads;
  const int win = bx % nwin, b = bx / nwin;
  const int wy = win / nwx, wx = win - wy * nwx;

  auto pixel = [&](int tok) { return window_pixel<WS>(wy, wx, tok, shift, H, W); };
  auto region = [&](int tok) { return window_region<WS>(wy, wx, tok, shift, H, W); };
  for (int kk = t; kk < NK; kk += 256) {
    if (OCA) {
      const int ky = kk / WSE, py = wy * WS - (WSE - WS) / 2 + ky, px = wx * WS - (WSE - WS) / 2 + (kk - ky * WSE);
      sKPix[kk] = (py >= 0 && py < H && px >= 0 && px < W) ? py * W + px : -1;
    } else {
      sKPix[kk] = pixel(kk);
      sKRid[kk] = region(kk);
    }
  }
  if (t < QB) {
    sQPix[t] = pixel(qb * QB + t);
    sQRid[t] = region(qb * QB + t);
  }
  __syncthreads();
  const size_t img = (size_t)b * H * W;
  const int r31 = lane & 31, h = lane >> 5;

  // q by token (lane = token: conflict-free transposed stores)
  {
    const int i = t & 31, d0 = (t >> 5) * 4;
    const float* row = qkv + (img + sQPix[i]) * 3 * C + head * hd;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int d = d0 + e;
      sQt[d * QB + i] = d < hd ? row[d] * scale : 0.f;
    }
  }
  // St[j][i] = sum_d k[j][d] q[i][d] + bias (+ mask), a chunk of keys at a time: wave w owns keys [32 w, 32 w + 32) of the chunk
  const float* bh = biasT + (size_t)head * NK * WT;
  for (int c0 = 0; c0 < NK; c0 += KC) {
    __syncthreads();   // the previous chunk's operand reads are done
    {
      const int jj = t & (KC - 1), d0 = (t >> 7) * 16;
      const int pix = c0 + jj < NK ? sKPix[c0 + jj] : -1;
      const float* row = qkv + (img + (pix < 0 ? 0 : pix)) * 3 * C + C + head * hd;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int d = d0 + e;
        sKV[d * KP + jj] = (pix >= 0 && d < hd) ? row[d] : 0.f;
      }
    }
    __syncthreads();
    const int j0 = c0 + wave * 32;
    if (j0 < NK) {
      f32x16 acc;   // not score_tile: this kernel compiles to other code with it
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
      for (int s = 0; s < HD / 2; ++s) {
        const int kr = 2 * s + h;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sKV[kr * KP + wave * 32 + r31], sQt[kr * QB + r31], acc, 0, 0, 0);
      }
      const int ri = sQRid[r31], qg = qb * QB + r31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = acc_row(j0, r, h);
        float v = acc[r] + bh[(size_t)j * WT + qg];
        if (!OCA && sKRid[j] != ri) v += -100.f;
        sSt[j * QB + r31] = v;
      }
    }
  }
  __syncthreads();
  // row softmax: thread (part, i) covers the keys j = part (mod 8) of query i; the eight partial results combine in order
  {
    const int i = t & 31, part = t >> 5;
    float m = sSt[part * QB + i];
    for (int j = part + 8; j < NK; j += 8) m = fmaxf(m, sSt[j * QB + i]);
    sRed[part * QB + i] = m;
    __syncthreads();
    m = sRed[i];
#pragma unroll
    for (int q = 1; q < 8; ++q) m = fmaxf(m, sRed[q * QB + i]);
    __syncthreads();
    float s = 0.f;
    for (int j = part; j < NK; j += 8) {
      const float e = expf(sSt[j * QB + i] - m);
      sSt[j * QB + i] = e;
      s += e;
    }
    sRed[part * QB + i] = s;
    __syncthreads();
    s = sRed[i];
#pragma unroll
    for (int q = 1; q < 8; ++q) s += sRed[q * QB + i];
    for (int j = part; j < NK; j += 8) sSt[j * QB + i] = sSt[j * QB + i] / s;
  }
  // O[i][d] = sum_j P[i][j] v[j][d], the keys in order (one chain per output): wave 0 owns the 32 queries
  f32x16 o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;
  for (int c0 = 0; c0 < NK; c0 += KC) {
    __syncthreads();   // the probabilities are written; the previous chunk's reads are done
    {
      const int d = t & 31;
#pragma unroll
      for (int e = 0; e < KC / 8; ++e) {
        const int jj = (t >> 5) + 8 * e;
        const int pix = c0 + jj < NK ? sKPix[c0 + jj] : -1;
        sKV[jj * HD + d] = (pix >= 0 && d < hd) ? qkv[(img + pix) * 3 * C + 2 * C + head * hd + d] : 0.f;
      }
    }
    __syncthreads();
    if (wave == 0) {
      const int n = NK - c0 < KC ? NK - c0 : KC;
      for (int s = 0; s < n / 2; ++s) {
        const int kr = 2 * s + h;
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(sSt[(c0 + kr) * QB + r31], sKV[kr * HD + r31], o, 0, 0, 0);
      }
    }
  }
  if (wave == 0 && r31 < hd) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * h;   // acc_row(0, r, h), written out: the call changes this kernel's code
      out[(img + sQPix[i]) * C + head * hd + r31] = o[r];
    }
  }
}

// the kinds HAT adds: RPB_OCA owns the tensor `name` itself (RPB is the bias table of the HABs' self-attention), GATE a 1x1
// Conv2d as the checkpoint holds it
enum HatKind { RPB_OCA = KIND_EXT, GATE };

struct LayerDesc : SwinLayerDesc<WS> {
  int tensors() const { return kind == RPB_OCA ? 1 : SwinLayerDesc::tensors(); }
  std::string tensor_name(int j) const { return kind == RPB_OCA ? name : SwinLayerDesc::tensor_name(j); }
  std::vector<int64_t> shape(int j) const {
    if (kind == RPB_OCA) return {(WS + WSE - 1) * (WS + WSE - 1), cout};
    if (kind == GATE && j == 0) return {cout, cin, 1, 1};
    return SwinLayerDesc::shape(j);
  }
};

struct Walker;

// what fdsr_swin_engine.h and fdsr_swin_walk.h need to know of this family
struct Hat : SwinFamily<WS> {
  using Config = fdsr_hat_config;
  using Desc = LayerDesc;
  using Walk = Walker;
  using Obj = fdsr_hat_obj;
  using Args = HatGemmArgs;
  static constexpr const char *name = "fdsr_hat", *graph_flag_name = "FDSR_HAT_GRAPH";
  static constexpr int NBUF = 10, graph_flag = FDSR_HAT_GRAPH;
  // no crop: the reference returns the padded size times the scale
  static int out_side(const Config&, int, int padded) { return padded; }

  // upsample.upsampling.{2,4}.* name the tensor of upsample.upsampling.0.* again (one Conv2d in every stage)
  static std::string canonical_name(const fdsr_hat_config& cfg, const char* name) {
    static const char prefix[] = "upsample.upsampling.";
    std::string nm(name);
    if (cfg.upscale == 3 || nm.compare(0, sizeof(prefix) - 1, prefix) != 0) return nm;
    const size_t dot = nm.find('.', sizeof(prefix) - 1);
    if (dot == std::string::npos) return nm;
    const std::string idx = nm.substr(sizeof(prefix) - 1, dot - (sizeof(prefix) - 1));
    for (int k = 1; (1 << k) < cfg.upscale; ++k)
      if (idx == std::to_string(2 * k)) return prefix + std::string("0") + nm.substr(dot);
    return nm;
  }

  // device: the common kinds as SwinFamily packs them; GATE as the checkpoint holds it; RPB_OCA biasT [heads][576 keys][256 queries]
  static void pack(const LayerDesc& L, int j, const float* host_f32, std::vector<float>& packed) {
    if (L.kind == RPB_OCA) {
      // relative_position_index_OCA is ((ky - qy) - 7) * 39 + ((kx - qx) - 7), -880 .. 640, and indexes a 1521-row table: the
      // negative values count from its end
      const int side = WS + WSE - 1, rows = side * side, off = WS - WSE + 1;
      packed.resize((size_t)L.cout * WKT * WT);
      for (int hh = 0; hh < L.cout; ++hh)
        for (int kj = 0; kj < WKT; ++kj)
          for (int qi = 0; qi < WT; ++qi) {
            int idx = ((kj / WSE) - (qi >> 4) + off) * side + ((kj % WSE) - (qi & 15) + off);
            if (idx < 0) idx += rows;
            packed[((size_t)hh * WKT + kj) * WT + qi] = host_f32[(size_t)idx * L.cout + hh];
          }
    } else if (L.kind == GATE) {
      packed.assign(host_f32, host_f32 + (j == 1 ? (size_t)L.cout : (size_t)L.cout * L.cin));
    } else {
      SwinFamily::pack(L, j, host_f32, packed);
    }
  }
};

struct Walker : SwinWalker<Hat> {
  int shared = -1;   // the layer of the upsampling convolution, once it has run

  // the GEMM kernels HAT adds, then the common ones
  void launch(int kind, int epi, const HatGemmArgs& a, bool vec) {
    if (kind == LINEAR && epi == EPI_HAB) check(launch_swin_gemm<ROWS, EPI_HAB>(a, vec, st));
    else if (kind == CONV && epi == EPI_GELU) check(launch_swin_gemm<CONV3, EPI_GELU>(static_cast<const GemmArgs&>(a), vec, st));
    else if (kind == CONV && epi == EPI_COLSUM) check(launch_swin_gemm<CONV3, EPI_COLSUM>(a, vec, st));
    else SwinWalker::launch(kind, epi, a, vec);
  }

  // attention over the q | k | v rows of `qkv`, into buffer 4
  T attention(const std::string& name, bool oca, const T& qkv, int heads, int shift) {
    return SwinWalker::attention(name, oca ? RPB_OCA : RPB, qkv, heads, 4, [&](const float* bias, int hd) {
      const int C = qkv.C / 3;
      const unsigned blocks = (unsigned)(N * (qkv.H / WS) * (qkv.W / WS) * heads * (WT / QB));
      const float scale = 1.f / sqrtf((float)hd);
      if (oca) hipLaunchKernelGGL(hat_attn_kernel<true>, dim3(blocks), dim3(256), 0, st, buf[qkv.buf], bias, buf[4], qkv.H, qkv.W, C, heads, hd, 0, scale);
      else hipLaunchKernelGGL(hat_attn_kernel<false>, dim3(blocks), dim3(256), 0, st, buf[qkv.buf], bias, buf[4], qkv.H, qkv.W, C, heads, hd, shift, scale);
    });
  }

  // the gate of `cab` [N][H][W][C] from its partial column sums (buffer 8), into buffer 9
  void gate(const std::string& name, const T& cab) {
    const int Cs = cab.C / cfg.squeeze_factor;
    const int i1 = layer(name + ".1", GATE, cab.C, Cs), i2 = layer(name + ".3", GATE, Cs, cab.C);
    if (mode == SIZE) {
      need[8] = std::max(need[8], (size_t)(cab.H * cab.W / 64) * cab.C);
      need[9] = std::max(need[9], (size_t)cab.C);
    }
    if (!live()) return;
    hipLaunchKernelGGL(hat_gate_kernel, dim3((unsigned)N), dim3(256), 0, st, buf[8], w[i1], b[i1], w[i2], b[i2], buf[9], cab.H * cab.W / 64, cab.C, Cs,
                       (float)(cab.H * cab.W));
    check(hipGetLastError());
  }

  // RHAG i: depth HABs (the odd ones on the shifted window), then one OCAB.  Buffers beyond the common ones: 6 / 7 the CAB's
  // hidden map and output, 8 its partial column sums, 9 the gate.
  T group(int i, const std::string& lp, T cur) {
    const std::string gp = lp + ".residual_group";
    const int C = cfg.embed_dim, heads = cfg.num_heads[i], Hp = cur.H, Wp = cur.W;
    for (int j = 0; j < cfg.depths[i]; ++j) {
      const std::string bp = gp + ".blocks." + std::to_string(j), tp = lp + ".blocks." + std::to_string(j);
      T n1 = norm(bp + ".norm1", cur, 4);
      T qkv = gemm(bp + ".attn.qkv", LINEAR, EPI_NONE, n1, 3 * C, 5);
      T mid = gemm(bp + ".conv_block.cab.0", CONV, EPI_GELU, n1, C / cfg.compress_ratio, 6);
      HatGemmArgs sums{}, hab{};
      sums.colsum = buf[8];
      T cab = gemm(bp + ".conv_block.cab.2", CONV, EPI_COLSUM, mid, C, 7, nullptr, 1, sums);
      gate(bp + ".conv_block.cab.3.attention", cab);
      if (stops_at(tp + ".cab")) {
        const size_t total = (size_t)N * Hp * Wp * C;
        hipLaunchKernelGGL(hat_gate_mul_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, buf[7], buf[9], buf[6], Hp * Wp, C, total);
        check(hipGetLastError());
      }
      if (mode == SIZE) touch(T{6, Hp, Wp, C});
      tap(tp + ".cab", T{6, Hp, Wp, C});
      T o = attention(bp + ".attn.relative_position_bias_table", false, qkv, heads, j % 2 ? WS / 2 : 0);
      hab.gate = buf[9];
      hab.cab = buf[cab.buf];
      hab.conv_scale = cfg.conv_scale;
      T y = gemm(bp + ".attn.proj", LINEAR, EPI_HAB, o, C, 3, &cur, 1, hab);
      tap(tp + ".attn", y);
      cur = mlp(bp, y);
      tap(tp + ".mlp", cur);
    }
    const std::string op = gp + ".overlap_attn";
    T n1 = norm(op + ".norm1", cur, 4);
    T qkv = gemm(op + ".qkv", LINEAR, EPI_NONE, n1, 3 * C, 5);
    T o = attention(op + ".relative_position_bias_table", true, qkv, heads, 0);
    T y = gemm(op + ".proj", LINEAR, EPI_RES, o, C, 3, &cur);
    tap(lp + ".ocab.attn", y);
    cur = mlp(op, y);
    tap(lp + ".ocab.mlp", cur);
    return cur;
  }

  // Upsample repeats ONE list of modules: the same Conv2d(64, 256) runs in every stage
  T upsample(int k, const T& y, int r, int ob) {
    reuse = k ? shared : -1;
    const T out = gemm("upsample.upsampling.0", CONV, EPI_SHUFFLE, y, r * r * NUM_FEAT, ob, nullptr, r);
    if (k == 0) shared = li - 1;
    return out;
  }
};

}  // namespace

struct fdsr_hat_obj : Engine<Hat> {};

extern "C" {

int fdsr_hat_create(const fdsr_hat_config* cfg, fdsr_hat* out) {
  if (!cfg || !out) return fail(nullptr, FDSR_E_INVALID, "fdsr_hat_create: null argument");
  const fdsr_hat_config& c = *cfg;
  const char* fn = "fdsr_hat_create";
  int rc;
  if ((rc = check_window(fn, c, WS))) return rc;
  if (c.overlap_win_size != WSE)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_hat_create: overlap window %d is not supported (24 only: overlap_ratio 0.5)", c.overlap_win_size);
  if ((rc = check_widths(fn, c, FDSR_HAT_MAX_LAYERS))) return rc;
  if (c.compress_ratio < 1 || c.embed_dim % c.compress_ratio)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_hat_create: embed_dim %d is not divisible by compress_ratio %d", c.embed_dim, c.compress_ratio);
  if (c.squeeze_factor < 1 || c.embed_dim / c.squeeze_factor < 1)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_hat_create: squeeze_factor %d leaves no channel of embed_dim %d", c.squeeze_factor, c.embed_dim);
  if ((rc = check_layers_and_output(fn, c))) return rc;
  return engine_create<Hat>(fn, c, out);
}

void fdsr_hat_destroy(fdsr_hat s) { engine_destroy<Hat>(s); }

int fdsr_hat_load(fdsr_hat s, const char* name, const float* host_f32, const int64_t* shape, int ndim) {
  return engine_load<Hat>("fdsr_hat_load", s, name, host_f32, shape, ndim);
}

int fdsr_hat_workspace_bytes(fdsr_hat s, int batch, int height, int width, size_t* bytes) {
  return engine_workspace_bytes<Hat>("fdsr_hat_workspace_bytes", s, batch, height, width, bytes);
}

int fdsr_hat_forward(fdsr_hat s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace, size_t workspace_bytes,
                     void* hip_stream, int flags) {
  return engine_forward<Hat>("fdsr_hat_forward", s, x_nchw, batch, height, width, out_nchw, workspace, workspace_bytes, hip_stream, flags);
}

int fdsr_hat_debug_tensor(fdsr_hat s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                          size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return engine_debug_tensor<Hat>("fdsr_hat_debug_tensor", s, name, x_nchw, batch, height, width, out_nhwc, capacity_floats, dims3, workspace,
                                  workspace_bytes, hip_stream);
}

}  // extern "C"
