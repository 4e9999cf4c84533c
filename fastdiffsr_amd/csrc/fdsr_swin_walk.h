// The host side of the window-transformer families (fdsr_swinir.hip, fdsr_hat.hip), written once on top of fdsr_swin_engine.h:
// the common tensor kinds and their packing, the reflect-pad shape check, the GEMM dispatcher, the walk of the network (head,
// residual groups, MLP half of a block, reconstruction tail) and the configuration checks the two fdsr_*_create share.
// A family writes `struct Walker : SwinWalker<F>` and adds to the traits of fdsr_swin_engine.h (F : SwinFamily<window side>):
//   Args                      its GEMM argument struct (GemmArgs, or a struct derived from it for added epilogues)
//   out_side(cfg, given, padded)  the side conv_last stores: the crop rule
// and to the walker:
//   group(i, lp, cur)         the blocks of residual group i (checkpoint prefix lp) from the tokens `cur`; returns the tokens
//   upsample(k, y, r, ob)     stage k of the pixel-shuffle upsampler: which convolution of the checkpoint it is
//   launch(kind, epi, a, vec) only where it adds GEMM kernels: its own rows first, then SwinWalker::launch.  A unit
//                             instantiates the kernels it launches and no other; the rows here run on GemmArgs in every unit.
// Nothing here asks which family it serves.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "fdsr_swin_engine.h"

namespace {

// KIND_EXT and above: kinds a family adds.  LINEAR / CONV / LNORM own name.weight and name.bias, RPB owns the tensor `name` itself
enum Kind { LINEAR, CONV, LNORM, RPB, KIND_EXT };

// One named module of the checkpoint
template <int WS>
struct SwinLayerDesc {
  std::string name;
  int kind;
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

// biasT[head][j][i] = table[(yi - yj + WS - 1) * (2 WS - 1) + (xi - xj + WS - 1)][head], key j and query i tokens of a WS x WS
// window: the gather of relative_position_index, once
template <int WS>
void pack_window_bias(int heads, const float* table, std::vector<float>& packed) {
  constexpr int WT = WS * WS;
  packed.resize((size_t)heads * WT * WT);
  for (int hh = 0; hh < heads; ++hh)
    for (int kj = 0; kj < WT; ++kj)
      for (int qi = 0; qi < WT; ++qi) {
        const int idx = (qi / WS - kj / WS + WS - 1) * (2 * WS - 1) + (qi % WS - kj % WS + WS - 1);
        packed[((size_t)hh * WT + kj) * WT + qi] = table[(size_t)idx * heads + hh];
      }
}

template <int WS>
struct SwinFamily : FamilyDefaults {
  static constexpr int SIDE = WS;

  // F.pad's rule for 'reflect': the padding must be smaller than the side it mirrors
  static int check_shape(const char* fn, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, B, H, W);
    const int ph = round_up(H, WS) - H, pw = round_up(W, WS) - W;
    if (ph >= H || pw >= W)
      return fail(nullptr, FDSR_E_INVALID, "%s: a %dx%d image cannot be reflect-padded by (%d, %d) to a multiple of the window", fn, H, W, ph, pw);
    return FDSR_OK;
  }

  // device: LINEAR / CONV packed [Kpad][Npad] + bias [Npad]; LNORM gamma + beta; RPB biasT [heads][WS WS keys][WS WS queries]
  template <class D>
  static void pack(const D& L, int j, const float* host_f32, std::vector<float>& packed) {
    if (L.kind == RPB) pack_window_bias<WS>(L.cout, host_f32, packed);
    else if (L.kind == LNORM) packed.assign(host_f32, host_f32 + L.cout);
    else pack_gemm_tensor(L.kind == CONV, j == 1, L.cin, L.cout, host_f32, packed);
  }
};

// The network, common to the families.  Buffers: 0 the packed input, 1 conv_first's output (kept for conv_after_body), 2 / 3 the
// tokens (a group's input stays in 2 while its blocks work in 3), 4 a LayerNorm's or an attention's output, 5 qkv / the MLP's
// hidden rows; the reconstruction tail alternates between 4 and 5.  6 and above are the family's.
template <class F>
struct SwinWalker : WalkerBase<F> {
  using B = WalkerBase<F>;
  using B::buf; using B::cfg; using B::check; using B::dst; using B::gemm_args; using B::Hin; using B::img; using B::layer; using B::live;
  using B::mode; using B::N; using B::norm; using B::st; using B::tap; using B::touch; using B::w; using B::Win;
  using Args = typename F::Args;
  static constexpr int WS = F::SIDE;
  typename F::Walk& self() { return static_cast<typename F::Walk&>(*this); }

  void launch(int kind, int epi, const GemmArgs& a, bool vec) {
    if (kind == LINEAR) {
      if (epi == EPI_NONE) check(launch_swin_gemm<ROWS, EPI_NONE>(a, vec, st));
      else if (epi == EPI_GELU) check(launch_swin_gemm<ROWS, EPI_GELU>(a, vec, st));
      else check(launch_swin_gemm<ROWS, EPI_RES>(a, vec, st));
    } else {
      if (epi == EPI_NONE) check(launch_swin_gemm<CONV3, EPI_NONE>(a, vec, st));
      else if (epi == EPI_LRELU) check(launch_swin_gemm<CONV3, EPI_LRELU>(a, vec, st));
      else if (epi == EPI_RES) check(launch_swin_gemm<CONV3, EPI_RES>(a, vec, st));
      else if (epi == EPI_SHUFFLE) check(launch_swin_gemm<CONV3, EPI_SHUFFLE>(a, vec, st));
      else check(launch_swin_gemm<CONV3, EPI_NCHW>(a, vec, st));
    }
  }

  // out = epilogue(gather(in) . W + bias).  res: the EPI_RES addend.  r: the EPI_SHUFFLE factor.  a: what an added epilogue reads.
  T gemm(const std::string& name, int kind, int epi, const T& in, int cout, int ob, const T* res = nullptr, int r = 1, Args a = Args{}) {
    const int idx = layer(name, kind, in.C, cout);
    T out{ob, in.H * r, in.W * r, cout / (r * r)};
    if (mode == SIZE && epi != EPI_NCHW) touch(out);
    if (!live()) return out;
    gemm_args(a, idx, in, res, kind == CONV, in.C, cout, r);
    a.out = epi == EPI_NCHW ? dst : buf[ob];
    a.Hc = F::out_side(cfg, Hin, in.H);
    a.Wc = F::out_side(cfg, Win, in.W);
    a.slope = 0.01f;   // nn.LeakyReLU()'s default
    a.range = cfg.img_range;
    for (int c = 0; c < 3; ++c) a.mean[c] = cfg.mean[c];
    self().launch(kind, epi, a, in.C % 4 == 0);
    return out;
  }

  T norm(const std::string& name, const T& in, int ob) { return norm(layer(name, LNORM, in.C, in.C), in, ob); }

  // attention over the q | k | v rows of `qkv`, into `ob`; run(bias, head_dim) launches the family's kernel
  template <class Run>
  T attention(const std::string& name, int kind, const T& qkv, int heads, int ob, Run run) {
    const int idx = layer(name, kind, 0, heads);
    const int C = qkv.C / 3;
    T out{ob, qkv.H, qkv.W, C};
    if (mode == SIZE) touch(out);
    if (!live()) return out;
    run(w[idx], C / heads);
    check(hipGetLastError());
    return out;
  }

  // y + fc2(gelu(fc1(norm2(y))))
  T mlp(const std::string& p, const T& y) {
    T n2 = norm(p + ".norm2", y, 4);
    T hid = gemm(p + ".mlp.fc1", LINEAR, EPI_GELU, n2, cfg.mlp_hidden, 5);
    return gemm(p + ".mlp.fc2", LINEAR, EPI_RES, hid, y.C, 3, &y);
  }

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
      const T cur = self().group(i, lp, a);
      a = gemm(lp + ".conv", CONV, EPI_RES, cur, C, 2, &a);
      tap(lp, a);
    }
    T n = norm("norm", a, 4);
    T y = gemm("conv_after_body", CONV, EPI_RES, n, C, 3, &f);
    tap("conv_after_body", y);
    y = gemm("conv_before_upsample.0", CONV, EPI_LRELU, y, NUM_FEAT, 4);
    // one conv + PixelShuffle(2) per factor of two, one conv + PixelShuffle(3) at scale 3
    const int r = cfg.upscale == 3 ? 3 : 2;
    int ob = 5;
    for (int k = 0, s = 1; s < cfg.upscale; ++k, s *= r, ob = 9 - ob) {
      y = self().upsample(k, y, r, ob);
      tap("upsample." + std::to_string(k), y);
    }
    gemm("conv_last", CONV, EPI_NCHW, y, 3, 0);
  }
};

// The checks of fdsr_*_create that the families share, in three runs: a family's own checks go between them
template <class C>
int check_window(const char* fn, const C& c, int ws) {
  if (c.window_size != ws) return fail(nullptr, FDSR_E_INVALID, "%s: window_size %d is not supported (%d only)", fn, c.window_size, ws);
  return FDSR_OK;
}

template <class C>
int check_widths(const char* fn, const C& c, int max_layers) {
  if (c.n_layers < 1 || c.n_layers > max_layers) return fail(nullptr, FDSR_E_INVALID, "%s: %d layers (1..%d)", fn, c.n_layers, max_layers);
  if (c.embed_dim < 1 || c.embed_dim > LN_MAX_C || c.mlp_hidden < 1)
    return fail(nullptr, FDSR_E_INVALID, "%s: embed_dim %d (1..%d), mlp hidden width %d", fn, c.embed_dim, LN_MAX_C, c.mlp_hidden);
  return FDSR_OK;
}

template <class C>
int check_layers_and_output(const char* fn, const C& c) {
  for (int i = 0; i < c.n_layers; ++i) {
    if (c.depths[i] < 1 || c.num_heads[i] < 1 || c.embed_dim % c.num_heads[i])
      return fail(nullptr, FDSR_E_INVALID, "%s: layer %d: depth %d, embed_dim %d over %d heads", fn, i, c.depths[i], c.embed_dim, c.num_heads[i]);
    if (c.embed_dim / c.num_heads[i] > HD)
      return fail(nullptr, FDSR_E_INVALID, "%s: layer %d: head_dim %d is not supported (at most %d)", fn, i, c.embed_dim / c.num_heads[i], HD);
  }
  if (c.upscale != 2 && c.upscale != 3 && c.upscale != 4 && c.upscale != 8)
    return fail(nullptr, FDSR_E_INVALID, "%s: upscale %d is not supported (2, 3, 4, 8)", fn, c.upscale);
  if (!(c.img_range > 0.f)) return fail(nullptr, FDSR_E_INVALID, "%s: img_range must be positive", fn);
  return FDSR_OK;
}

}  // namespace
