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
// The network is written once, as a walk: the same code lists the checkpoint tensors in load order, sizes the workspace and
// launches the kernels.  The walk, its GEMM dispatcher, the tensor kinds and the shape and configuration checks are
// fdsr_swin_walk.h's, shared with HAT; this file holds SwinIR's kernels, its Swin block (Walker::group), its naming of the
// upsampling convolutions, its traits and its extern "C" functions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fdsr_engine_int.h"
#include "fdsr_swin_common.h"   // swin_gemm_kernel, swin_ln_kernel, swin_input_kernel, the attention pieces, the weight packing
#include "fdsr_swin_engine.h"   // the walk's bookkeeping, the engine object and the frames of the C functions
#include "fdsr_swin_walk.h"     // the window-transformer walk

using namespace fdsr_int;

namespace {

constexpr int WS = 8, WT = WS * WS;   // the window and its tokens
constexpr int TP = WT + 32;           // pitch of the [k][token] operand arrays of the attention kernel

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
    sPix[t] = window_pixel<WS>(wy, wx, t, shift, H, W);
    sRid[t] = window_region<WS>(wy, wx, t, shift, H, W);
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
      f32x16 acc;   // not score_tile: this kernel compiles to other code with it
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
        const int j = acc_row(wj * 32, r, h);
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
          const int i = acc_row(wave * 32, r, h);
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

using LayerDesc = SwinLayerDesc<WS>;

struct Walker;

// what fdsr_swin_engine.h and fdsr_swin_walk.h need to know of this family
struct Swinir : SwinFamily<WS> {
  using Config = fdsr_swinir_config;
  using Desc = LayerDesc;
  using Walk = Walker;
  using Obj = fdsr_swinir_obj;
  using Args = GemmArgs;
  static constexpr const char *name = "fdsr_swinir", *graph_flag_name = "FDSR_SWINIR_GRAPH";
  static constexpr int NBUF = 6, graph_flag = FDSR_SWINIR_GRAPH;
  // the reference crops to the input's size times the scale
  static int out_side(const Config& cfg, int given, int) { return given * cfg.upscale; }
};

struct Walker : SwinWalker<Swinir> {
  // RSTB i: depth Swin blocks, the odd ones on the window shifted by half its side
  T group(int i, const std::string& lp, T cur) {
    const int C = cfg.embed_dim;
    for (int j = 0; j < cfg.depths[i]; ++j) {
      const std::string bp = lp + ".residual_group.blocks." + std::to_string(j), tp = lp + ".blocks." + std::to_string(j);
      T n1 = norm(bp + ".norm1", cur, 4);
      T qkv = gemm(bp + ".attn.qkv", LINEAR, EPI_NONE, n1, 3 * C, 5);
      const int shift = j % 2 ? WS / 2 : 0;
      T o = attention(bp + ".attn.relative_position_bias_table", RPB, qkv, cfg.num_heads[i], 4, [&](const float* bias, int hd) {
        const unsigned blocks = (unsigned)(N * (qkv.H / WS) * (qkv.W / WS));
        hipLaunchKernelGGL(swin_attn_kernel, dim3(blocks), dim3(256), 0, st, buf[qkv.buf], bias, buf[4], qkv.H, qkv.W, C, cfg.num_heads[i], hd, shift,
                           1.f / sqrtf((float)hd));
      });
      T y = gemm(bp + ".attn.proj", LINEAR, EPI_RES, o, C, 3, &cur);
      tap(tp + ".attn", y);
      cur = mlp(bp, y);
      tap(tp + ".mlp", cur);
    }
    return cur;
  }

  // a convolution of its own per stage: upsample.0, upsample.2, upsample.4
  T upsample(int k, const T& y, int r, int ob) {
    return gemm("upsample." + std::to_string(2 * k), CONV, EPI_SHUFFLE, y, r * r * NUM_FEAT, ob, nullptr, r);
  }
};

}  // namespace

struct fdsr_swinir_obj : Engine<Swinir> {};

extern "C" {

int fdsr_swinir_create(const fdsr_swinir_config* cfg, fdsr_swinir* out) {
  if (!cfg || !out) return fail(nullptr, FDSR_E_INVALID, "fdsr_swinir_create: null argument");
  const char* fn = "fdsr_swinir_create";
  int rc;
  if ((rc = check_window(fn, *cfg, WS)) || (rc = check_widths(fn, *cfg, FDSR_SWINIR_MAX_LAYERS)) || (rc = check_layers_and_output(fn, *cfg))) return rc;
  return engine_create<Swinir>(fn, *cfg, out);
}

void fdsr_swinir_destroy(fdsr_swinir s) { engine_destroy<Swinir>(s); }

int fdsr_swinir_load(fdsr_swinir s, const char* name, const float* host_f32, const int64_t* shape, int ndim) {
  return engine_load<Swinir>("fdsr_swinir_load", s, name, host_f32, shape, ndim);
}

int fdsr_swinir_workspace_bytes(fdsr_swinir s, int batch, int height, int width, size_t* bytes) {
  return engine_workspace_bytes<Swinir>("fdsr_swinir_workspace_bytes", s, batch, height, width, bytes);
}

int fdsr_swinir_forward(fdsr_swinir s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace,
                        size_t workspace_bytes, void* hip_stream, int flags) {
  return engine_forward<Swinir>("fdsr_swinir_forward", s, x_nchw, batch, height, width, out_nchw, workspace, workspace_bytes, hip_stream, flags);
}

int fdsr_swinir_debug_tensor(fdsr_swinir s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                             size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return engine_debug_tensor<Swinir>("fdsr_swinir_debug_tensor", s, name, x_nchw, batch, height, width, out_nhwc, capacity_floats, dims3, workspace,
                                     workspace_bytes, hip_stream);
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
