// TransENet (MSI_SR_model/model/transenet.py: TransENet, model/transformer.py) inference in exact fp32 on gfx950.
//
//   x     = sub_mean(img)                            a general 3x3 matrix + bias, NCHW -> NHWC       transenet_input_kernel
//   f     = head(x);   s_i = five ResBlocks(f), i = 1, 2, 3 (each from f; conv, ReLU, conv, + x; no outer skip)
//   u     = pixel_shuffle(conv(.)) per factor of two on s_3, a convolution of its own per stage (one conv + PixelShuffle(3) at 3)
//   l_i   = stage{i}_conv1x1(s_i);  h = up_conv1x1(u)                                     n_feats -> channels = n_feats / 4
//   t     = patch_to_embedding(8 x 8 x channels patches, K index (p1 8 + p2) channels + c) -> 512       the PATCH8 gather
//   four encoders (en_depth layers): t += to_out(attention(to_qkv(LN t)));  t += W2 gelu_tanh(W1 LN t)
//   three decoders on the high tokens, decoder3(., e_3), decoder2(., e_2), decoder1(., e_1) (de_depth layers):
//           self-attention as above; t += to_out(attention(to_q(LN t), to_k(LN m), to_v(LN m))), ONE LayerNorm; feed-forward
//   y     = embedding_to_patch(t) stored straight to its NHWC pixels (EPI_SCATTER); span_conv1x1; tail; add_mean, NHWC -> NCHW
//
// The token GEMM, its 3x3 gather, LayerNorm, the weight packing and the attention kernel's score tile, row map and chunk sizes
// (QB, KC, KP) are fdsr_swin_common.h's.  New here:
//   transenet_attn_kernel  dense attention of 6 heads of 32 over every token: one workgroup per (image, head, 32 queries), k and v
//                          streamed through LDS in chunks of 128 keys in order, LDS independent of Nk.  Two passes that both
//                          form S^T on the MFMA: the first keeps the row maxima, the second writes exp(s - max) of a chunk to
//                          LDS, adds it to the row sums and runs P V on four 16 x 16 tiles (v_mfma_f32_16x16x4_f32, one per
//                          wave: a k-ordered chain per output); the quotient by the row sum comes last.  No rescaling.
//   three GEMM epilogues   EPI_RELU, EPI_GELUT (the tanh form), EPI_SCATTER (the inverse patch rearrange as a store address).
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

constexpr int DIM = 512, HEADS = 6, INNER = HEADS * HD, MLP = 512, PS = 8;   // hard-coded inside the reference's __init__

enum TransEpi { EPI_RELU = EPI_EXT, EPI_GELUT = EPI_EXT + 1, EPI_SCATTER = EPI_EXT + 2 };

template <int EPI, class ARGS>
__device__ void gemm_epilogue_ext(const ARGS& p, const f32x16 (&acc)[2], int row0, int co, int h, float bias) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int om = acc_row(row0 + mb * 32, i, h);
      if (om >= p.M) continue;
      const float v = acc[mb][i] + bias;
      if constexpr (EPI == EPI_RELU) {
        p.out[(size_t)om * p.N + co] = fmaxf(v, 0.f);
      } else if constexpr (EPI == EPI_GELUT) {
        p.out[(size_t)om * p.N + co] = 0.5f * v * (1.f + tanhf(0.79788456080286535588f * (v + 0.044715f * v * v * v)));
      } else {
        // EPI_SCATTER: column co = (p1 8 + p2) Cin + c of token (b, ty, tx) is channel c of pixel (ty 8 + p1, tx 8 + p2) of the
        // NHWC map [B][H][W][Cin]
        const int pp = co / p.Cin, c = co - pp * p.Cin, p1 = pp >> 3, p2 = pp & 7;
        const int tw = p.W / PS, ntok = (p.H / PS) * tw;
        const int b = om / ntok, tk = om - b * ntok, ty = tk / tw, tx = tk - ty * tw;
        p.out[(((size_t)b * p.H + ty * PS + p1) * p.W + tx * PS + p2) * p.Cin + c] = v;
      }
    }
}

// [B][3][H][W] -> NHWC [B][H][W][3], y = A x + b: sub_mean as the checkpoint holds it (A [3][3] row-major, out x in)
__global__ void __launch_bounds__(256) transenet_input_kernel(const float* __restrict__ x, const float* __restrict__ A, const float* __restrict__ bias,
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
__global__ void __launch_bounds__(256) transenet_output_kernel(const float* __restrict__ x, const float* __restrict__ A, const float* __restrict__ bias,
                                                               float* __restrict__ y, int HW, size_t pixels) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const size_t b = i / HW, pix = i - b * HW;
  const float v0 = x[i * 3], v1 = x[i * 3 + 1], v2 = x[i * 3 + 2];
#pragma unroll
  for (int c = 0; c < 3; ++c) y[(b * 3 + c) * HW + pix] = A[c * 3] * v0 + A[c * 3 + 1] * v1 + A[c * 3 + 2] * v2 + bias[c];
}

// Attention of one (image, head, block of QB queries): O[i][d] = sum_j softmax_j(scale q_i . k_j) v[j][d], d < 32.
// q / k / v: row (b Nq + i) or (b Nk + j) of a GEMM output with row stride qs / ks / vs floats, already at the column where q, k
// or v begins; the head's 32 columns follow at head * 32.  Row strides and column offsets are multiples of 4 floats.
// Keys >= Nk of the last chunk are zero rows that enter neither the max nor the sum (their e is 0, as is their v); queries >= Nq
// are zero rows that are not stored.
__global__ void __launch_bounds__(256) transenet_attn_kernel(const float* __restrict__ q, int qs, const float* __restrict__ k, int ks,
                                                             const float* __restrict__ v, int vs, float* __restrict__ out, int os, int Nq, int Nk,
                                                             float scale) {
  __shared__ __attribute__((aligned(16))) float sQt[HD * QB];   // [d][query], q * scale
  __shared__ __attribute__((aligned(16))) float sK[HD * KP];    // [d][key] of the chunk
  __shared__ __attribute__((aligned(16))) float sV[KC * HD];    // [key][d] of the chunk
  __shared__ __attribute__((aligned(16))) float sSt[KC * QB];   // [key][query]: exp(s - max) of the chunk
  __shared__ float sRed[4 * QB];
  __shared__ float sM[QB], sL[QB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nqb = (Nq + QB - 1) / QB;
  int bx = blockIdx.x;
  const int qb = bx % nqb;
  bx /= nqb;
  const int head = bx % HEADS, b = bx / HEADS;
  const int q0 = qb * QB;
  const int r31 = lane & 31, h = lane >> 5;
  const float* kb = k + (size_t)b * Nk * ks + head * HD;
  const float* vb = v + (size_t)b * Nk * vs + head * HD;

  {
    const int i = t & 31, d0 = (t >> 5) * 4;
    f32x4 qv = {0.f, 0.f, 0.f, 0.f};
    if (q0 + i < Nq) qv = *reinterpret_cast<const f32x4*>(q + ((size_t)b * Nq + q0 + i) * qs + head * HD + d0);
#pragma unroll
    for (int e = 0; e < 4; ++e) sQt[(d0 + e) * QB + i] = qv[e] * scale;
  }

  auto stage_k = [&](int c0) {
    const int jj = t & (KC - 1), d0 = (t >> 7) * 16;
    const bool ok = c0 + jj < Nk;
    const float* row = kb + (size_t)(ok ? c0 + jj : 0) * ks + d0;
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      f32x4 kv = {0.f, 0.f, 0.f, 0.f};
      if (ok) kv = *reinterpret_cast<const f32x4*>(row + 4 * e4);
#pragma unroll
      for (int e = 0; e < 4; ++e) sK[(d0 + 4 * e4 + e) * KP + jj] = kv[e];
    }
  };
  // St[j][i] of this wave's 32 keys of the chunk: row j = acc_row(32 wave, r, h), column i = r31
  auto scores = [&]() { return score_tile(sK, KP, wave * 32, sQt, QB, 0, r31, h); };

  // pass 1: the row maxima
  float m = -INFINITY;
  for (int c0 = 0; c0 < Nk; c0 += KC) {
    __syncthreads();   // the previous chunk's operand reads are done (first: sQt is written)
    stage_k(c0);
    __syncthreads();
    const f32x16 acc = scores();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = acc_row(c0 + wave * 32, r, h);
      if (j < Nk) m = fmaxf(m, acc[r]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (h == 0) sRed[wave * QB + r31] = m;
  __syncthreads();
  if (t < QB) sM[t] = fmaxf(fmaxf(sRed[t], sRed[QB + t]), fmaxf(sRed[2 * QB + t], sRed[3 * QB + t]));
  __syncthreads();
  m = sM[r31];

  // pass 2: e = exp(s - max), the row sums, O += e v with the keys in order
  const int qi = wave & 1, dj = wave >> 1, l15 = lane & 15, l4 = lane >> 4;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  float lsum = 0.f;
  for (int c0 = 0; c0 < Nk; c0 += KC) {
    __syncthreads();   // the previous chunk's reads of sK, sV and sSt are done
    stage_k(c0);
    {
      const int d = t & 31;
#pragma unroll
      for (int e = 0; e < KC / 8; ++e) {
        const int jj = (t >> 5) + 8 * e;
        sV[jj * HD + d] = c0 + jj < Nk ? vb[(size_t)(c0 + jj) * vs + d] : 0.f;
      }
    }
    __syncthreads();
    const f32x16 acc = scores();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jl = acc_row(wave * 32, r, h);
      const float e = c0 + jl < Nk ? expf(acc[r] - m) : 0.f;
      lsum += e;
      sSt[jl * QB + r31] = e;
    }
    __syncthreads();
    // 16x16x4 operands: A[i = lane & 15][k = lane >> 4] (query, key), B[k = lane >> 4][j = lane & 15] (key, d)
    const int n = Nk - c0 < KC ? Nk - c0 : KC;
    for (int s = 0; s < (n + 3) / 4; ++s) {
      const int kr = 4 * s + l4;
      o = __builtin_amdgcn_mfma_f32_16x16x4f32(sSt[kr * QB + qi * 16 + l15], sV[kr * HD + dj * 16 + l15], o, 0, 0, 0);
    }
  }
  // the row sums: this lane's keys, the other half of the wave, then the four waves in order
  lsum += __shfl_xor(lsum, 32, 64);
  if (h == 0) sRed[wave * QB + r31] = lsum;
  __syncthreads();
  if (t < QB) sL[t] = ((sRed[t] + sRed[QB + t]) + sRed[2 * QB + t]) + sRed[3 * QB + t];
  __syncthreads();
  // C/D map of 16x16x4: column = lane & 15 (d), row = 4 (lane >> 4) + r (query)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = qi * 16 + 4 * l4 + r;
    if (q0 + i < Nq) out[((size_t)b * Nq + q0 + i) * os + head * HD + dj * 16 + l15] = o[r] / sL[i];
  }
}

enum Kind { LINEAR, LINEAR_NB, CONV, CONV1, LNORM, MEAN };

// One named module of the checkpoint: name.weight and name.bias (LINEAR_NB: the weight alone)
struct LayerDesc {
  std::string name;
  Kind kind;
  int cin, cout;   // LNORM: cout = C
  int tensors() const { return kind == LINEAR_NB ? 1 : 2; }
  std::string tensor_name(int j) const { return name + (j == 0 ? ".weight" : ".bias"); }
  std::vector<int64_t> shape(int j) const {
    if (j == 1 || kind == LNORM) return {cout};
    if (kind == CONV) return {cout, cin, 3, 3};
    if (kind == CONV1 || kind == MEAN) return {cout, cin, 1, 1};
    return {cout, cin};
  }
};

struct Walker;

// what fdsr_swin_engine.h needs to know of this family
struct Transenet : FamilyDefaults {
  using Config = fdsr_transenet_config;
  using Desc = LayerDesc;
  using Walk = Walker;
  using Obj = fdsr_transenet_obj;
  static constexpr const char *name = "fdsr_transenet", *graph_flag_name = "FDSR_TRANSENET_GRAPH";
  static constexpr int NBUF = 18, SIDE = PS, graph_flag = FDSR_TRANSENET_GRAPH;

  static int check_shape(const char* fn, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, B, H, W);
    if (H % PS || W % PS) return fail(nullptr, FDSR_E_INVALID, "%s: a %dx%d image is not made of 8 x 8 patches (both sides must be multiples of 8)", fn, H, W);
    if ((long long)B * H * W * 64 > (1ll << 30)) return fail(nullptr, FDSR_E_INVALID, "%s: %d images of %dx%d are too many pixels for one call", fn, B, H, W);
    return FDSR_OK;
  }

  // device: LINEAR / LINEAR_NB / CONV / CONV1 packed [Kpad][Npad] + bias [Npad] (LINEAR_NB: zeros); LNORM gamma + beta; MEAN as the checkpoint holds it
  static void pack(const LayerDesc& L, int j, const float* host_f32, std::vector<float>& packed) {
    if (L.kind == LNORM) packed.assign(host_f32, host_f32 + L.cout);
    else if (L.kind == MEAN) packed.assign(host_f32, host_f32 + (j == 1 ? 3 : 9));
    else pack_gemm_tensor(L.kind == CONV, j == 1, L.cin, L.cout, host_f32, packed);
  }

  // bias=False: the GEMM adds a row of zeros
  static int after_load(Engine<Transenet>& s, int layer) {
    const LayerDesc& L = s.table[layer];
    if (L.kind != LINEAR_NB || s.b[layer]) return FDSR_OK;
    const size_t bytes = (size_t)gemm_npad(L.cout) * sizeof(float);
    HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&s.b[layer]), bytes));
    HIPCHK(nullptr, hipMemset(s.b[layer], 0, bytes));
    return FDSR_OK;
  }
};

struct Walker : WalkerBase<Transenet> {
  // out = epilogue(gather(in) . W + bias).  res: the EPI_RES addend (may be the output).  r: the EPI_SHUFFLE factor.
  // patch: the rows are the 8 x 8 x C patches of `in`.
  T gemm(const std::string& name, Kind kind, int epi, const T& in, int cout, int ob, const T* res = nullptr, int r = 1, bool patch = false) {
    const int cin = patch ? PS * PS * in.C : in.C;
    const int idx = layer(name, kind, cin, cout);
    T out{ob, in.H * r, in.W * r, cout / (r * r)};
    if (patch) out = T{ob, in.H / PS, in.W / PS, cout};
    if (epi == EPI_SCATTER) out = T{ob, in.H * PS, in.W * PS, cout / (PS * PS)};
    if (mode == SIZE) touch(out);
    if (!live()) return out;
    GemmArgs a{};
    gemm_args(a, idx, in, res, kind == CONV, cin, cout, r);
    a.out = buf[ob];
    if (patch) a.M = N * out.H * out.W;
    if (epi == EPI_SCATTER) a.H = out.H, a.W = out.W, a.Cin = out.C;
    const bool vec = in.C % 4 == 0;
    if (patch) {
      check(launch_swin_gemm<PATCH8, EPI_NONE>(a, vec, st));
    } else if (kind == CONV) {
      if (epi == EPI_NONE) check(launch_swin_gemm<CONV3, EPI_NONE>(a, vec, st));
      else if (epi == EPI_RELU) check(launch_swin_gemm<CONV3, EPI_RELU>(a, vec, st));
      else if (epi == EPI_RES) check(launch_swin_gemm<CONV3, EPI_RES>(a, vec, st));
      else check(launch_swin_gemm<CONV3, EPI_SHUFFLE>(a, vec, st));
    } else {
      if (epi == EPI_NONE) check(launch_swin_gemm<ROWS, EPI_NONE>(a, vec, st));
      else if (epi == EPI_RES) check(launch_swin_gemm<ROWS, EPI_RES>(a, vec, st));
      else if (epi == EPI_GELUT) check(launch_swin_gemm<ROWS, EPI_GELUT>(a, vec, st));
      else check(launch_swin_gemm<ROWS, EPI_SCATTER>(a, vec, st));
    }
    return out;
  }

  // softmax(scale q k^T) v over all tokens of an image, into buffer 15; the logit scale is dim ** -0.5, as the reference has it
  T attention(const T& q, int qoff, const T& k, int koff, const T& v, int voff) {
    T out{15, q.H, q.W, INNER};
    if (mode == SIZE) touch(out);
    if (!live()) return out;
    const int Nq = q.H * q.W, Nk = k.H * k.W;
    const unsigned blocks = (unsigned)(N * HEADS * ((Nq + QB - 1) / QB));
    hipLaunchKernelGGL(transenet_attn_kernel, dim3(blocks), dim3(256), 0, st, buf[q.buf] + qoff, q.C, buf[k.buf] + koff, k.C, buf[v.buf] + voff, v.C,
                       buf[15], INNER, Nq, Nk, 1.f / sqrtf((float)DIM));
    check(hipGetLastError());
    return out;
  }

  // Residual(PreNorm(Attention)): x += to_out(attention(to_qkv(LN x))), in place
  void self_block(const std::string& p, const T& x) {
    const T n = norm(layer(p + ".fn.norm", LNORM, DIM, DIM), x, 13);
    const T qkv = gemm(p + ".fn.fn.to_qkv", LINEAR_NB, EPI_NONE, n, 3 * INNER, 14);
    const T o = attention(qkv, 0, qkv, INNER, qkv, 2 * INNER);
    gemm(p + ".fn.fn.to_out.0", LINEAR, EPI_RES, o, DIM, x.buf, &x);
  }
  // Residual2(PreNorm2(MixedAttention)): q from x, k and v from m, both through the same LayerNorm
  void cross_block(const std::string& p, const T& x, const T& m) {
    const int ln = layer(p + ".fn.norm", LNORM, DIM, DIM);
    const T n = norm(ln, x, 13);
    const T q = gemm(p + ".fn.fn.to_q", LINEAR_NB, EPI_NONE, n, INNER, 14);
    const T nm = norm(ln, m, 13);
    const T k = gemm(p + ".fn.fn.to_k", LINEAR_NB, EPI_NONE, nm, INNER, 16);
    const T v = gemm(p + ".fn.fn.to_v", LINEAR_NB, EPI_NONE, nm, INNER, 17);
    const T o = attention(q, 0, k, 0, v, 0);
    gemm(p + ".fn.fn.to_out.0", LINEAR, EPI_RES, o, DIM, x.buf, &x);
  }
  void ff_block(const std::string& p, const T& x) {
    const T n = norm(layer(p + ".fn.norm", LNORM, DIM, DIM), x, 13);
    const T hid = gemm(p + ".fn.fn.net.0", LINEAR, EPI_GELUT, n, MLP, 14);
    gemm(p + ".fn.fn.net.3", LINEAR, EPI_RES, hid, DIM, x.buf, &x);
  }

  void mean_shift(const char* name, bool input, const T& t) {
    const int idx = layer(name, MEAN, 3, 3);
    if (!live() || (!input && !dst)) return;
    const size_t pixels = (size_t)N * t.H * t.W;
    const dim3 grid((unsigned)((pixels + 255) / 256));
    if (input) hipLaunchKernelGGL(transenet_input_kernel, grid, dim3(256), 0, st, img, w[idx], b[idx], buf[t.buf], t.H * t.W, pixels);
    else hipLaunchKernelGGL(transenet_output_kernel, grid, dim3(256), 0, st, buf[t.buf], w[idx], b[idx], dst, t.H * t.W, pixels);
    check(hipGetLastError());
  }

  // The whole network.  Buffers: 0 the input after sub_mean, 1 head's output, 2 / 3 / 4 the maps of the stages, the upsampler and
  // the tail, 5 / 6 / 7 the stages' 1x1 outputs, 8 the high 1x1 output and later embedding_to_patch's map, 9 / 10 / 11 the low
  // tokens, 12 the high tokens, 13 a LayerNorm's output, 14 qkv / q / the hidden rows, 15 an attention's output, 16 / 17 the
  // cross-attention's k and v.
  void walk() {
    const int nf = cfg.n_feats, ch = nf / 4, H = std::max(Hin, PS), W = std::max(Win, PS);
    T x{0, H, W, 3};
    if (mode == SIZE) touch(x);
    mean_shift("sub_mean", true, x);
    const T f = gemm("head.0", CONV, EPI_NONE, x, nf, 1);
    tap("head", f);
    T low[3], s3{};
    for (int s = 1; s <= 3; ++s) {
      const std::string sp = "feat_extrat_stage" + std::to_string(s), tn = "stage" + std::to_string(s);
      T cur = f;
      for (int i = 0; i < 5; ++i) {
        const std::string bp = sp + ".body." + std::to_string(i) + ".body.";
        const T t = gemm(bp + "0", CONV, EPI_RELU, cur, nf, 4);
        cur = gemm(bp + "2", CONV, EPI_RES, t, nf, cur.buf == 2 ? 3 : 2, &cur);
      }
      tap(tn, cur);
      low[s - 1] = gemm(tn + "_conv1x1", CONV1, EPI_NONE, cur, ch, 4 + s);
      tap(tn + ".1x1", low[s - 1]);
      s3 = cur;
    }
    T u = s3;
    if (cfg.scale == 3) {
      u = gemm("upsampler.0", CONV, EPI_SHUFFLE, u, 9 * nf, u.buf == 2 ? 3 : 2, nullptr, 3);
    } else {
      for (int k = 0; (1 << k) < cfg.scale; ++k) u = gemm("upsampler." + std::to_string(2 * k), CONV, EPI_SHUFFLE, u, 4 * nf, u.buf == 2 ? 3 : 2, nullptr, 2);
    }
    tap("up", u);
    const T hi = gemm("up_conv1x1", CONV1, EPI_NONE, u, ch, 8);
    tap("up.1x1", hi);

    T tok[4];
    for (int s = 0; s < 3; ++s) {
      tok[s] = gemm("patch_to_embedding_low" + std::to_string(s + 1), LINEAR, EPI_NONE, low[s], DIM, 9 + s, nullptr, 1, true);
      tap("embed.low" + std::to_string(s + 1), tok[s]);
    }
    tok[3] = gemm("patch_to_embedding_high", LINEAR, EPI_NONE, hi, DIM, 12, nullptr, 1, true);
    tap("embed.high", tok[3]);

    static const char* const enc[4] = {"encoder_stage1", "encoder_stage2", "encoder_stage3", "encoder_up"};
    for (int e = 0; e < 4; ++e) {
      for (int j = 0; j < cfg.en_depth; ++j) {
        const std::string lp = std::string(enc[e]) + ".layers." + std::to_string(j), tp = std::string(enc[e]) + "." + std::to_string(j);
        self_block(lp + ".0", tok[e]);
        tap(tp + ".attn", tok[e]);
        ff_block(lp + ".1", tok[e]);
        tap(tp + ".ff", tok[e]);
      }
      tap(enc[e], tok[e]);
    }
    const T y = tok[3];
    for (int d = 3; d >= 1; --d) {
      const std::string dn = "decoder" + std::to_string(d);
      for (int j = 0; j < cfg.de_depth; ++j) {
        const std::string lp = dn + ".layers." + std::to_string(j), tp = dn + "." + std::to_string(j);
        self_block(lp + ".0", y);
        tap(tp + ".self", y);
        cross_block(lp + ".1", y, tok[d - 1]);
        tap(tp + ".cross", y);
        ff_block(lp + ".2", y);
        tap(tp + ".ff", y);
      }
    }
    const T pm = gemm("embedding_to_patch", LINEAR, EPI_SCATTER, y, PS * PS * ch, 8);
    tap("embedding_to_patch", pm);
    const T sp = gemm("span_conv1x1", CONV1, EPI_NONE, pm, nf, 2);
    tap("span", sp);
    const T tl = gemm("tail", CONV, EPI_NONE, sp, 3, 3);
    mean_shift("add_mean", false, tl);
  }
};

}  // namespace

struct fdsr_transenet_obj : Engine<Transenet> {};

extern "C" {

int fdsr_transenet_create(const fdsr_transenet_config* cfg, fdsr_transenet* out) {
  if (!cfg || !out) return fail(nullptr, FDSR_E_INVALID, "fdsr_transenet_create: null argument");
  const fdsr_transenet_config& c = *cfg;
  if (c.n_colors != 3) return fail(nullptr, FDSR_E_INVALID, "fdsr_transenet_create: n_colors %d is not supported (3 only)", c.n_colors);
  if (c.n_feats < 16 || c.n_feats > 256 || c.n_feats % 16)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_transenet_create: n_feats %d is not supported (a multiple of 16, 16..256)", c.n_feats);
  if (c.scale != 2 && c.scale != 3 && c.scale != 4 && c.scale != 8)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_transenet_create: scale %d is not supported (2, 3, 4, 8)", c.scale);
  if (c.en_depth < 1 || c.en_depth > FDSR_TRANSENET_MAX_DEPTH)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_transenet_create: en_depth %d (1..%d)", c.en_depth, FDSR_TRANSENET_MAX_DEPTH);
  if (c.de_depth < 1 || c.de_depth > FDSR_TRANSENET_MAX_DEPTH)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_transenet_create: de_depth %d (1..%d)", c.de_depth, FDSR_TRANSENET_MAX_DEPTH);
  return engine_create<Transenet>("fdsr_transenet_create", c, out);
}

void fdsr_transenet_destroy(fdsr_transenet s) { engine_destroy<Transenet>(s); }

int fdsr_transenet_load(fdsr_transenet s, const char* name, const float* host_f32, const int64_t* shape, int ndim) {
  return engine_load<Transenet>("fdsr_transenet_load", s, name, host_f32, shape, ndim);
}

int fdsr_transenet_workspace_bytes(fdsr_transenet s, int batch, int height, int width, size_t* bytes) {
  return engine_workspace_bytes<Transenet>("fdsr_transenet_workspace_bytes", s, batch, height, width, bytes);
}

int fdsr_transenet_forward(fdsr_transenet s, const float* x_nchw, int batch, int height, int width, float* out_nchw, void* workspace,
                           size_t workspace_bytes, void* hip_stream, int flags) {
  return engine_forward<Transenet>("fdsr_transenet_forward", s, x_nchw, batch, height, width, out_nchw, workspace, workspace_bytes, hip_stream, flags);
}

int fdsr_transenet_debug_tensor(fdsr_transenet s, const char* name, const float* x_nchw, int batch, int height, int width, float* out_nhwc,
                                size_t capacity_floats, int* dims3, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return engine_debug_tensor<Transenet>("fdsr_transenet_debug_tensor", s, name, x_nchw, batch, height, width, out_nhwc, capacity_floats, dims3,
                                        workspace, workspace_bytes, hip_stream);
}

}  // extern "C"
