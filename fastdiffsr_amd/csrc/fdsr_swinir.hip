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
#include "fdsr_swin_common.h"   // swin_gemm_kernel, swin_ln_kernel, swin_input_kernel, the weight packing
#include "fdsr_swin_engine.h"   // the walk's bookkeeping, the engine object and the frames of the C functions

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
  int tensors() const { return kind == RPB ? 1 : 2; }
  std::string tensor_name(int j) const { return kind == RPB ? name : name + (j == 0 ? ".weight" : ".bias"); }
  std::vector<int64_t> shape(int j) const {
    if (kind == RPB) return {(2 * WS - 1) * (2 * WS - 1), cout};
    if (j == 1 || kind == LNORM) return {cout};
    if (kind == CONV) return {cout, cin, 3, 3};
    return {cout, cin};
  }
};

struct Walker;

// what fdsr_swin_engine.h needs to know of this family
struct Swinir : FamilyDefaults {
  using Config = fdsr_swinir_config;
  using Desc = LayerDesc;
  using Walk = Walker;
  using Obj = fdsr_swinir_obj;
  static constexpr const char *name = "fdsr_swinir", *graph_flag_name = "FDSR_SWINIR_GRAPH";
  static constexpr int NBUF = 6, SIDE = WS, graph_flag = FDSR_SWINIR_GRAPH;

  // F.pad's rule for 'reflect': the padding must be smaller than the side it mirrors
  static int check_shape(const char* fn, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, B, H, W);
    const int ph = round_up(H, WS) - H, pw = round_up(W, WS) - W;
    if (ph >= H || pw >= W)
      return fail(nullptr, FDSR_E_INVALID, "%s: a %dx%d image cannot be reflect-padded by (%d, %d) to a multiple of the window", fn, H, W, ph, pw);
    return FDSR_OK;
  }

  // device: LINEAR / CONV packed [Kpad][Npad] + bias [Npad]; LNORM gamma + beta; RPB biasT [heads][64][64]
  static void pack(const LayerDesc& L, int j, const float* host_f32, std::vector<float>& packed) {
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
    } else {
      pack_gemm_tensor(L.kind == CONV, j == 1, L.cin, L.cout, host_f32, packed);
    }
  }
};

struct Walker : WalkerBase<Swinir> {
  template <int GATHER, int EPI>
  void launch_gemm(const GemmArgs& a, bool vec) {
    check(launch_swin_gemm<GATHER, EPI>(a, vec, st));
  }

  // out = epilogue(gather(in) . W + bias).  res: the EPI_RES addend.  r: the EPI_SHUFFLE factor.
  T gemm(const std::string& name, Kind kind, int epi, const T& in, int cout, int ob, const T* res = nullptr, int r = 1) {
    const int idx = layer(name, kind, in.C, cout);
    T out{ob, in.H * r, in.W * r, cout / (r * r)};
    if (mode == SIZE && epi != EPI_NCHW) touch(out);
    if (!live()) return out;
    GemmArgs a{};
    gemm_args(a, idx, in, res, kind == CONV, in.C, cout, r);
    a.out = epi == EPI_NCHW ? dst : buf[ob];
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

  using WalkerBase::norm;
  T norm(const std::string& name, const T& in, int ob) { return norm(layer(name, LNORM, in.C, in.C), in, ob); }

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

}  // namespace

struct fdsr_swinir_obj : Engine<Swinir> {};

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
  return engine_create<Swinir>("fdsr_swinir_create", c, out);
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
