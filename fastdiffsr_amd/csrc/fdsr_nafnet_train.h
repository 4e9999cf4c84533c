// EDiffSR training on gfx950: one step of DenoisingModel.optimize_parameters (EDiffSR/codes/config/sisr/models/denoising_model.py) for
// ConditionalNAFNet + IR-SDE, fp32.  Part of fdsr_nafnet.hip's translation unit (it shares the forward kernels, the schema and Run).
//
//   forward          Run::net itself, the walk sampling runs, over another destination table (train_dst): every tensor the backward
//                    reads lands in a slot of its own instead of one of sampling's four shared buffers, and conv4 keeps its pair
//   loss head        xt_1_expection, xt_1_optimum, MatchingLoss (l1 / l2), d eps
//   backward         input gradients: naf_gemm_kernel over the transposed packs (pack_forms); weight / bias gradients:
//                    naf_wgrad_kernel (v_mfma_f32_32x32x2_f32, split over pixel chunks, second pass in chunk order); the rest elementwise
//   optimizer        Adam / AdamW / Lion over the flat master, then a gather re-pack of every device form
//
// No atomics anywhere: every sum has one order, fixed by the shapes alone.  Kept per block: out, LN statistics, conv1's output, the
// gated product, the SCA vector, y, conv4's pair before the gate and its product.  Recomputed in the backward: the LN-modulated
// inputs of conv1 / conv4 and the SCA-scaled input of conv3 (prologues of the weight-gradient kernel), conv2's outputs (in the gate's
// backward), conv3's and conv5's outputs (for d beta / d gamma), SCA's and the RCAB's pooled means.
//
// f16 training storage (fdsr_nafnet_set_train_storage; the contract is in include/fdsr.h): the forward is fdsr_nafnet_h1.h's into
// half-size slots, and every backward kernel that reads a saved activation is a template on the stored type (ACT_F32 / ACT_F16 through
// fdsr_act_io.h's ActIO): it widens what it reads, which is exact, and computes in fp32 as before.  Gradients stay fp32 everywhere.

namespace {

constexpr int ACT_F32 = fdsr::PREC_F16X3, ACT_F16 = fdsr::PREC_F16;   // ActIO's names for fp32 and f16 elements in memory
template <int ST>
__device__ __forceinline__ float act_ld(const float* base, size_t i) { return fdsr::ActIO<ST>::load1(base, i); }

constexpr int WG_CHUNK = 2048;   // pixels per partial sum of a weight gradient
constexpr int WG_PB = 16;        // pixels per LDS stage
constexpr int WG_P = 64 + 32;    // LDS pitch, as AP / BP

struct WgArgs {
  const float* x;        // the convolution's input, NHWC [N][Hin][Win][Cin]
  const float* dy;       // [M][ldy] gradient of its output
  const float* stats;    // PRO_LN
  const float* pmul;     // PRO_MUL / PRO_LN, image n at pmul + n * pstride
  const float* padd;
  const float* colmul;   // dy[.][co] *= colmul[co] (beta / gamma), or null
  float* part;           // [nz][KP][CP]
  int N, Hin, Win, Cin, Hout, Wout, Cout, KW, S, P, K, Keff, ldy, pstride;
};

// dW[k][co] = sum over pixels of A[p][k] dY[p][co]; A is the forward GEMM's operand (im2col, with the forward's prologue), and
// row k == K (when Keff > K) is a column of ones: the bias gradient.  Workgroup: 64 k x 64 co of one pixel chunk; wave w owns the
// 32 x 32 tile (w & 1, w >> 1).  MFMA 32x32x2: A[i = k][kk = pixel], B[kk = pixel][j = co]; 16 pixels per stage.
// XS / DS: the stored type of x / dy (dy is a saved activation only for ups, whose operands are exchanged).  Where x is f16 and a
// prologue forms A again, A is clamped and rounded to f16 as the forward staged it: dW is the derivative of the product the forward
// computed.
template <int PRO, int XS, int DS>
__global__ void __launch_bounds__(256) naf_wgrad_kernel(WgArgs p) {
  __shared__ float sA[WG_PB * WG_P];
  __shared__ float sB[WG_PB * WG_P];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int kl = t & 63, pl0 = t >> 6;
  const int HWo = p.Hout * p.Wout, M = p.N * HWo;
  const int k = blockIdx.x * 64 + kl, co = blockIdx.y * 64 + kl;
  const bool kval = k < p.K, kone = k >= p.K && k < p.Keff, cval = co < p.Cout;
  int ci = 0, ky = 0, kx = 0;
  if (kval) {
    const int tap = k / p.Cin;
    ci = k - tap * p.Cin;
    ky = tap / p.KW;
    kx = tap - ky * p.KW;
  }
  const float cm = (cval && p.colmul) ? p.colmul[co] : 1.f;
  const int pbeg = blockIdx.z * WG_CHUNK, pend = min(M, pbeg + WG_CHUNK);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int r31 = lane & 31, h = lane >> 5, kh = wave & 1, ch = wave >> 1;
  for (int p0 = pbeg; p0 < pend; p0 += WG_PB) {
    float ra[4], rb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pix = p0 + pl0 + 4 * j;
      float a = 0.f, b = 0.f;
      if (pix < pend) {
        if (cval) b = act_ld<DS>(p.dy, (size_t)pix * p.ldy + co) * cm;
        if (kone) a = 1.f;
        else if (kval) {
          const int n = pix / HWo, r = pix - n * HWo;
          const int oy = r / p.Wout, ox = r - oy * p.Wout;
          const int iy = oy * p.S - p.P + ky, ix = ox * p.S - p.P + kx;
          if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) {
            a = act_ld<XS>(p.x, (((size_t)n * p.Hin + iy) * p.Win + ix) * p.Cin + ci);
            if (PRO == PRO_MUL) a = naf_pro<PRO_MUL>(a, 0.f, 0.f, p.pmul[(size_t)n * p.pstride + ci], 0.f);
            if (PRO == PRO_LN)
              a = naf_pro<PRO_LN>(a, p.stats[2 * (size_t)pix], p.stats[2 * (size_t)pix + 1], p.pmul[(size_t)n * p.pstride + ci], p.padd[(size_t)n * p.pstride + ci]);
            if (XS == ACT_F16 && PRO != PRO_NONE) a = (float)(_Float16)__builtin_amdgcn_fmed3f(a, -F16_MAX, F16_MAX);
          }
        }
      }
      ra[j] = a;
      rb[j] = b;
    }
    __syncthreads();   // the previous stage's LDS reads are done
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sA[(pl0 + 4 * j) * WG_P + kl] = ra[j];
      sB[(pl0 + 4 * j) * WG_P + kl] = rb[j];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < WG_PB / 2; ++s) {
      const int pr = 2 * s + h;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[pr * WG_P + 32 * kh + r31], sB[pr * WG_P + 32 * ch + r31], acc, 0, 0, 0);
    }
  }
  // C/D map: column (co) = lane & 31, row (k) = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
  const int KP = gridDim.x * 64, CP = gridDim.y * 64;
  float* dst = p.part + ((size_t)blockIdx.z * KP + blockIdx.x * 64 + 32 * kh + 4 * h) * CP + blockIdx.y * 64 + 32 * ch + r31;
#pragma unroll
  for (int i = 0; i < 16; ++i) dst[(size_t)((i & 3) + 8 * (i >> 2)) * CP] = acc[i];
}

// the chunks in order, into the reference's layout.  mode 0: weight[co][ci][ky][kx] (k = tap Cin + ci), bias[co] (k == K);
// mode 1 (ups, operands exchanged): k = tap C' + c' is the output channel 4 c' + tap, the column is the input channel.
__global__ void __launch_bounds__(256) naf_wgrad_finish_kernel(const float* __restrict__ part, int nz, int KP, int CP, int Keff, int K, int Cout,
                                                               int Cin, int taps, int mode, float* __restrict__ gw, float* __restrict__ gb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Keff * Cout) return;
  const int k = i / Cout, co = i - k * Cout;
  float s = 0.f;
  for (int z = 0; z < nz; ++z) s += part[((size_t)z * KP + k) * CP + co];
  if (k >= K) { gb[co] = s; return; }
  const int tap = k / Cin, ci = k - tap * Cin;
  if (mode == 0) gw[((size_t)co * Cin + ci) * taps + tap] = s;
  else gw[(size_t)(4 * ci + tap) * Cout + co] = s;
}

// per-strip channel sums of a (mode 0), a b (mode 1) or a (b - mean) rstd (mode 2): part[n][strip][ch], as naf_chansum_kernel
template <int AS, int BS>
__global__ void __launch_bounds__(256) naf_dot_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ stats,
                                                      float* __restrict__ part, int HW, int c, int nstrips, int mode) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, py = threadIdx.x >> 6;
  const int ch = blockIdx.y * 64 + cl, n = blockIdx.z, strip = blockIdx.x;
  float sum = 0.f;
  if (ch < c)
    for (int q = py; q < STRIP; q += 4) {
      const int pix = strip * STRIP + q;
      if (pix >= HW) break;
      const size_t gp = (size_t)n * HW + pix, i = gp * c + ch;
      float v = act_ld<AS>(a, i);
      if (mode == 1) v *= act_ld<BS>(b, i);
      if (mode == 2) v *= (act_ld<BS>(b, i) - stats[2 * gp]) * stats[2 * gp + 1];
      sum += v;
    }
  red[py][cl] = sum;
  __syncthreads();
  if (py == 0 && ch < c) part[((size_t)n * nstrips + strip) * c + ch] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// dst[g][ch] = scale * (part[g G][ch] + part[g G + 1][ch] + ...), in order
__global__ void __launch_bounds__(256) naf_reduce_kernel(const float* __restrict__ part, float* __restrict__ dst, int groups, int G, int c, float scale,
                                                         int dstride) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= groups * c) return;
  const int g = i / c, ch = i - g * c;
  float s = 0.f;
  for (int k = 0; k < G; ++k) s += part[((size_t)g * G + k) * c + ch];
  dst[(size_t)g * dstride + ch] = s * scale;
}

// LayerNorm + FiLM backward onto the running gradient: out = xh mul + add, xh = (x - mean) rstd;
// g += rstd (d mul - mean_c(d mul) - xh mean_c(d mul xh)).  16 lanes per pixel, as naf_ln_stats_kernel.
template <int XS>
__global__ void __launch_bounds__(256) naf_ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ d, const float* __restrict__ stats,
                                                         const float* __restrict__ mul, int mstride, float* __restrict__ g, int M, int HW, int C) {
  const int sub = threadIdx.x & 15;
  const int pix = blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool ok = pix < M;
  const size_t base = (size_t)(ok ? pix : 0) * C;
  const float* m = mul + (size_t)((ok ? pix : 0) / HW) * mstride;
  const float mean = stats[2 * (size_t)(ok ? pix : 0)], rstd = stats[2 * (size_t)(ok ? pix : 0) + 1];
  float s1 = 0.f, s2 = 0.f;
  for (int c = sub; c < C; c += 16) {
    const float dh = d[base + c] * m[c], xh = (act_ld<XS>(x, base + c) - mean) * rstd;
    s1 += dh;
    s2 += dh * xh;
  }
#pragma unroll
  for (int o = 8; o; o >>= 1) { s1 += __shfl_xor(s1, o, 16); s2 += __shfl_xor(s2, o, 16); }
  s1 /= (float)C;
  s2 /= (float)C;
  if (!ok) return;
  for (int c = sub; c < C; c += 16) {
    const float dh = d[base + c] * m[c], xh = (act_ld<XS>(x, base + c) - mean) * rstd;
    g[base + c] += rstd * (dh - s1 - xh * s2);
  }
}

// SimpleGate backward from the saved pair: out[p][j] = d[p][j] u[p][c + j], out[p][c + j] = d[p][j] u[p][j]
template <int US>
__global__ void __launch_bounds__(256) naf_gate_bwd_kernel(const float* __restrict__ d, const float* __restrict__ u, float* __restrict__ out, int c,
                                                           size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t pix = i / c;
  const int j = (int)(i - pix * c);
  const float v = d[i];
  out[pix * 2 * c + j] = v * act_ld<US>(u, pix * 2 * c + c + j);
  out[pix * 2 * c + c + j] = v * act_ld<US>(u, pix * 2 * c + j);
}

// x sca backward, then conv2's SimpleGate: d t2 = d[p][ch] sca[n][ch] + dpool[n][ch]; conv2's two outputs are formed again from x.
template <int XS>
__global__ void __launch_bounds__(256) naf_dwgate_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                             const float* __restrict__ d, const float* __restrict__ sca, const float* __restrict__ dpool,
                                                             float* __restrict__ out, int H, int W, int c, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t gp = i / c;
  const int ch = (int)(i - gp * c), HW = H * W, C2 = 2 * c;
  const int n = (int)(gp / HW), pix = (int)(gp - (size_t)n * HW);
  const int yy = pix / W, xx = pix - yy * W;
  const float* xn = XS == ACT_F16 ? x + (size_t)n * HW * c : x + (size_t)n * HW * C2;   // the image (C2 halves are c floats)
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int iy = yy + dy - 1, ix = xx + dx - 1;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const size_t src = ((size_t)iy * W + ix) * C2;
      a0 += w[(dy * 3 + dx) * C2 + ch] * act_ld<XS>(xn, src + ch);
      a1 += w[(dy * 3 + dx) * C2 + c + ch] * act_ld<XS>(xn, src + c + ch);
    }
  a0 += b[ch];
  a1 += b[c + ch];
  const float dt2 = d[i] * sca[(size_t)n * c + ch] + dpool[(size_t)n * c + ch];
  out[gp * C2 + ch] = dt2 * a1;
  out[gp * C2 + c + ch] = dt2 * a0;
}

// depthwise 3x3 backward: dx[q][ch] = sum_k w[k][ch] da[q - off_k][ch]; and the strip's sums of da[p] x[p + off_k] (k < 9) and of da
// (k = 9): part[n][strip][10][C2]
template <int XS>
__global__ void __launch_bounds__(256) naf_dw_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ da,
                                                         float* __restrict__ dx, float* __restrict__ part, int H, int W, int C2, int nstrips) {
  __shared__ float red[4][10][64];
  const int cl = threadIdx.x & 63, py = threadIdx.x >> 6;
  const int ch = blockIdx.y * 64 + cl, n = blockIdx.z, strip = blockIdx.x;
  const int HW = H * W;
  float acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.f;
  if (ch < C2) {
    float wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = w[k * C2 + ch];
    const float* xn = XS == ACT_F16 ? x + (size_t)n * HW * (C2 / 2) : x + (size_t)n * HW * C2;   // the image (C2 is even)
    const float* dn = da + (size_t)n * HW * C2;
    for (int q = py; q < STRIP; q += 4) {
      const int pix = strip * STRIP + q;
      if (pix >= HW) break;
      const int yy = pix / W, xx = pix - yy * W;
      const float dv = dn[(size_t)pix * C2 + ch];
      float s = 0.f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dxx = 0; dxx < 3; ++dxx) {
          const int k = dy * 3 + dxx;
          const int fy = yy + dy - 1, fx = xx + dxx - 1;   // the forward tap of this pixel
          if (fy >= 0 && fy < H && fx >= 0 && fx < W) acc[k] += dv * act_ld<XS>(xn, ((size_t)fy * W + fx) * C2 + ch);
          const int by = yy - dy + 1, bx = xx - dxx + 1;   // the output pixel that read this one through tap k
          if (by >= 0 && by < H && bx >= 0 && bx < W) s += wk[k] * dn[((size_t)by * W + bx) * C2 + ch];
        }
      acc[9] += dv;
      dx[((size_t)n * HW + pix) * C2 + ch] = s;
    }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) red[py][k][cl] = acc[k];
  __syncthreads();
  if (py == 0 && ch < C2)
#pragma unroll
    for (int k = 0; k < 10; ++k)
      part[(((size_t)n * nstrips + strip) * 10 + k) * C2 + ch] = ((red[0][k][cl] + red[1][k][cl]) + red[2][k][cl]) + red[3][k][cl];
}

__global__ void __launch_bounds__(256) naf_dw_finish_kernel(const float* __restrict__ part, int G, int C2, float* __restrict__ gw, float* __restrict__ gb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 10 * C2) return;
  const int k = i / C2, ch = i - k * C2;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += part[((size_t)g * 10 + k) * C2 + ch];
  if (k < 9) gw[(size_t)ch * 9 + k] = s;
  else gb[ch] = s;
}

// SCA's mat-vec backward: dW[co][ci] = sum_n ds[n][co] pooled[n][ci], db[co] = sum_n ds[n][co]
__global__ void __launch_bounds__(256) naf_sca_bwd_w_kernel(const float* __restrict__ ds, const float* __restrict__ pooled, float* __restrict__ gw,
                                                            float* __restrict__ gb, int N, int c) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)c * c) return;
  const int co = (int)(i / c), ci = (int)(i - (size_t)co * c);
  float s = 0.f, sb = 0.f;
  for (int n = 0; n < N; ++n) {
    s += ds[(size_t)n * c + co] * pooled[(size_t)n * c + ci];
    sb += ds[(size_t)n * c + co];
  }
  gw[i] = s;
  if (ci == 0) gb[co] = sb;
}

// dpool[n][ci] = (sum_co W[co][ci] ds[n][co]) / HW: what every pixel of the pooled tensor receives
__global__ void __launch_bounds__(256) naf_sca_bwd_x_kernel(const float* __restrict__ ds, const float* __restrict__ w, float* __restrict__ dpool, int N,
                                                            int c, float inv_hw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * c) return;
  const int n = i / c, ci = i - n * c;
  float s = 0.f;
  for (int co = 0; co < c; ++co) s += w[(size_t)co * c + ci] * ds[(size_t)n * c + co];
  dpool[i] = s * inv_hw;
}

// RCAB's ChannelAttention backward, one block per image: pooled and hid are formed again; da [N][c] is sum_p d r.
// Writes dz2 [N][c], dz1 [N][cs], hid [N][cs], pooled [N][c] for the weight gradients and dpool [N][c] (divided by HW).
__global__ void __launch_bounds__(256) naf_ca_bwd_kernel(const float* __restrict__ part, int nstrips, int HW, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ att,
                                                         const float* __restrict__ da, float* __restrict__ dz2o, float* __restrict__ dz1o,
                                                         float* __restrict__ hido, float* __restrict__ pooledo, float* __restrict__ dpool, int c, int cs) {
  extern __shared__ float lds[];
  float* pooled = lds;
  float* tmp = lds + c;
  float* hid = tmp + 256;
  float* dz2 = hid + cs;
  float* dz1 = dz2 + c;
  const int n = blockIdx.x;
  pooled_to_lds(part, n, nstrips, HW, c, pooled, tmp);
  for (int j = threadIdx.x; j < cs; j += 256) {
    float a = b1[j];
    for (int ci = 0; ci < c; ++ci) a += w1[(size_t)j * c + ci] * pooled[ci];
    hid[j] = fmaxf(a, 0.f);
  }
  for (int co = threadIdx.x; co < c; co += 256) {
    const float a = att[(size_t)n * c + co];
    dz2[co] = da[(size_t)n * c + co] * a * (1.f - a);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < cs; j += 256) {
    float s = 0.f;
    for (int co = 0; co < c; ++co) s += w2[(size_t)co * cs + j] * dz2[co];
    dz1[j] = hid[j] > 0.f ? s : 0.f;
  }
  __syncthreads();
  for (int ci = threadIdx.x; ci < c; ci += 256) {
    float s = 0.f;
    for (int j = 0; j < cs; ++j) s += w1[(size_t)j * c + ci] * dz1[j];
    dpool[(size_t)n * c + ci] = s / (float)HW;
    dz2o[(size_t)n * c + ci] = dz2[ci];
    pooledo[(size_t)n * c + ci] = pooled[ci];
  }
  for (int j = threadIdx.x; j < cs; j += 256) {
    dz1o[(size_t)n * cs + j] = dz1[j];
    hido[(size_t)n * cs + j] = hid[j];
  }
}

// dW[r][j] = sum_b dr[b][r] in[b][j], db[r] = sum_b dr[b][r]: the gradients of a Linear / 1x1 on per-image vectors
__global__ void __launch_bounds__(256) naf_linear_w_kernel(const float* __restrict__ dr, const float* __restrict__ in, float* __restrict__ gw,
                                                           float* __restrict__ gb, int N, int R, int K) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)R * K) return;
  const int r = (int)(i / K), j = (int)(i - (size_t)r * K);
  float s = 0.f, sb = 0.f;
  for (int b = 0; b < N; ++b) {
    s += dr[(size_t)b * R + r] * in[(size_t)b * K + j];
    sb += dr[(size_t)b * R + r];
  }
  gw[i] = s;
  if (j == 0) gb[r] = sb;
}

// enhance: out = g a[n][ch] + dpool[n][ch]
__global__ void __launch_bounds__(256) naf_scale_add_kernel(const float* __restrict__ g, const float* __restrict__ a, const float* __restrict__ dpool,
                                                            float* __restrict__ out, int HW, int c, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % c);
  const size_t n = i / ((size_t)HW * c);
  out[i] = g[i] * a[n * c + ch] + dpool[n * c + ch];
}

template <int YS>
__global__ void __launch_bounds__(256) naf_relu_mask_kernel(float* __restrict__ g, const float* __restrict__ y, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total && !(act_ld<YS>(y, i) > 0.f)) g[i] = 0.f;
}

// g = 2 g + t: x + (rcab(x) + x) passes its gradient to x twice
__global__ void __launch_bounds__(256) naf_twice_plus_kernel(float* __restrict__ g, const float* __restrict__ t, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) g[i] = 2.f * g[i] + t[i];
}

// The blocks' Linear(2w, 4c) backward, one thread per row r.  In: drows[b][r] = the gradient of the FOLDED row (shift, or
// (scale + 1) g).  Unfolds: d g[ch] = sum_b d[b] (raw[b] + 1), d raw[b] = d[b] g[ch]; then d bias, d W[r][:].  drows becomes d raw.
// rowmap: [3][R] flat indices of W[r][0], bias[r] and g[ch] (-1 on shift rows).
__global__ void __launch_bounds__(256) naf_rows_bwd_kernel(const float* __restrict__ tg, const float* __restrict__ wT, const float* __restrict__ bias,
                                                           const float* __restrict__ mul, const int* __restrict__ rowmap, float* __restrict__ drows,
                                                           float* __restrict__ grad, int N, int K, int R) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int iw = rowmap[r], ib = rowmap[R + r], ig = rowmap[2 * R + r];
  float dg = 0.f, db = 0.f;
  for (int b = 0; b < N; ++b) {
    float d = drows[(size_t)b * R + r];
    if (ig >= 0) {
      float a = 0.f;
      for (int j = 0; j < K; ++j) a += wT[(size_t)j * R + r] * tg[(size_t)b * K + j];
      dg += d * ((a + bias[r]) + 1.f);
      d *= mul[r];
      drows[(size_t)b * R + r] = d;
    }
    db += d;
  }
  if (ig >= 0) grad[ig] = dg;
  grad[ib] = db;
  for (int j = 0; j < K; ++j) {
    float s = 0.f;
    for (int b = 0; b < N; ++b) s += drows[(size_t)b * R + r] * tg[(size_t)b * K + j];
    grad[iw + j] = s;
  }
}

// dtg[b][j] = sum_r draw[b][r] W[r][j]; one block per (j, b), a fixed tree over 256 interleaved partial sums
__global__ void __launch_bounds__(256) naf_dtg_kernel(const float* __restrict__ drows, const float* __restrict__ wT, float* __restrict__ dtg, int K, int R) {
  __shared__ float red[256];
  const int j = blockIdx.x, b = blockIdx.y;
  float s = 0.f;
  for (int r = threadIdx.x; r < R; r += 256) s += drows[(size_t)b * R + r] * wT[(size_t)j * R + r];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) dtg[(size_t)b * K + j] = red[0];
}

// time_mlp backward for one time value: the forward of naf_time_kernel again, then back to d h2 [4w], g1 [4w], d h1 [8w], emb [w]
__global__ void __launch_bounds__(256) naf_time_bwd_kernel(const float* __restrict__ time, const float* __restrict__ freq, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                           const float* __restrict__ dtg, float* __restrict__ dh2o, float* __restrict__ g1o,
                                                           float* __restrict__ dh1o, float* __restrict__ embo, int wd) {
  extern __shared__ float lds[];
  float* emb = lds;            // [wd]
  float* h1 = emb + wd;        // [8 wd]
  float* g1 = h1 + 8 * wd;     // [4 wd]
  float* h2 = g1 + 4 * wd;     // [4 wd]
  float* dh2 = h2 + 4 * wd;    // [4 wd]
  const int b = blockIdx.x, half = wd / 2;
  const float tv = time[b];
  for (int j = threadIdx.x; j < wd; j += 256) {
    const float a = __fmul_rn(tv, freq[j < half ? j : j - half]);
    emb[j] = j < half ? sinf(a) : cosf(a);
  }
  __syncthreads();
  for (int r = threadIdx.x; r < 8 * wd; r += 256) {
    float a = 0.f;
    for (int j = 0; j < wd; ++j) a += w1[(size_t)r * wd + j] * emb[j];
    h1[r] = a + b1[r];
  }
  __syncthreads();
  for (int r = threadIdx.x; r < 4 * wd; r += 256) g1[r] = h1[r] * h1[r + 4 * wd];
  __syncthreads();
  for (int r = threadIdx.x; r < 4 * wd; r += 256) {
    float a = 0.f;
    for (int j = 0; j < 4 * wd; ++j) a += w2[(size_t)r * 4 * wd + j] * g1[j];
    h2[r] = a + b2[r];
  }
  __syncthreads();
  for (int r = threadIdx.x; r < 2 * wd; r += 256) {
    const float d = dtg[(size_t)b * 2 * wd + r];
    dh2[r] = d * h2[r + 2 * wd];
    dh2[r + 2 * wd] = d * h2[r];
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 4 * wd; j += 256) {
    float s = 0.f;
    for (int r = 0; r < 4 * wd; ++r) s += w2[(size_t)r * 4 * wd + j] * dh2[r];
    dh1o[(size_t)b * 8 * wd + j] = s * h1[j + 4 * wd];
    dh1o[(size_t)b * 8 * wd + 4 * wd + j] = s * h1[j];
    dh2o[(size_t)b * 4 * wd + j] = dh2[j];
    g1o[(size_t)b * 4 * wd + j] = g1[j];
  }
  for (int j = threadIdx.x; j < wd; j += 256) embo[(size_t)b * wd + j] = emb[j];
}

__global__ void naf_i2f_kernel(const int* __restrict__ t, float* __restrict__ f, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) f[i] = (float)t[i];
}

struct LossTables { const float *theta, *sigma, *sbar, *cum; float dt; int T; };

// The loss head on the cropped image.  Per element, rounded operations in the reference's order:
//   expect = x - (theta (mu - x) - sigma^2 (-eps / sbar)) dt;  optimum = term1 (x - mu) + term2 (x0 - mu) + mu
// term1, term2 (reverse_optimum_step's A, B, C) are evaluated per image in fp64 from the fp32 tables and rounded once: 1 - B^2 cancels
// at small t, where an fp32 evaluation is only good to ~1e-5.  Writes d eps (padded NHWC; the border stays zero) and the block's sum
// of |diff| or diff^2 (a fixed tree) to part[n][block].
__global__ void __launch_bounds__(256) naf_loss_kernel(const float* __restrict__ eps, const float* __restrict__ x, const float* __restrict__ mu,
                                                       const float* __restrict__ x0, const int* __restrict__ tt, LossTables tb, int l2, float gscale,
                                                       float* __restrict__ deps, float* __restrict__ part, int H, int W, int Hp, int Wp) {
  __shared__ float red[256];
  const int n = blockIdx.y, HW = H * W;
  int t = tt[n];
  t = t < 1 ? 1 : t > tb.T ? tb.T : t;
  const float theta = tb.theta[t], sigma = tb.sigma[t], sbar = tb.sbar[t];
  const double dt = (double)tb.dt;
  const double A = exp(-(double)theta * dt), B = exp(-(double)tb.cum[t] * dt), C = exp(-(double)tb.cum[t - 1] * dt);
  const float term1 = (float)(A * (1.0 - C * C) / (1.0 - B * B)), term2 = (float)(C * (1.0 - A * A) / (1.0 - B * B));
  const float s2 = __fmul_rn(sigma, sigma);
  const float dexp = -(s2 / sbar) * tb.dt;   // d expect / d eps
  float sum = 0.f;
  for (int q = 0; q < 4; ++q) {
    const int pix = (blockIdx.x * 4 + q) * 256 + threadIdx.x;
    if (pix >= HW) break;
    const int py = pix / W, px = pix - py * W;
    const size_t ei = (((size_t)n * Hp + py) * Wp + px) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t si = ((size_t)n * 3 + c) * HW + pix;
      const float xv = x[si], m = mu[si];
      const float score = __fdiv_rn(-eps[ei + c], sbar);
      const float drift = __fmul_rn(__fsub_rn(__fmul_rn(theta, __fsub_rn(m, xv)), __fmul_rn(s2, score)), tb.dt);
      const float expect = __fsub_rn(xv, drift);
      const float opt = __fadd_rn(__fadd_rn(__fmul_rn(term1, __fsub_rn(xv, m)), __fmul_rn(term2, __fsub_rn(x0[si], m))), m);
      const float diff = __fsub_rn(expect, opt);
      float dl;
      if (l2) { sum += diff * diff; dl = 2.f * diff; }
      else { sum += fabsf(diff); dl = diff > 0.f ? 1.f : diff < 0.f ? -1.f : 0.f; }
      deps[ei + c] = dl * gscale * dexp;
    }
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)n * gridDim.x + blockIdx.x] = red[0];
}

// loss_out[1 + n] = mean over C H W of image n (its blocks in order); loss_out[0] = weight * mean over the images (in order)
__global__ void naf_loss_finish_kernel(const float* __restrict__ part, int nblk, int N, float inv_chw, float weight, float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float tot = 0.f;
  for (int n = 0; n < N; ++n) {
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += part[(size_t)n * nblk + k];
    s *= inv_chw;
    out[1 + n] = s;
    tot += s;
  }
  out[0] = weight * (tot / (float)N);
}

// The autograd bridge's two ends.  naf_dout_kernel: the caller's d out (NCHW, H x W) into the padded NHWC d eps slot, zero where
// the forward's crop dropped the prediction -- the place naf_loss_kernel's d eps takes in a built-in step.
__global__ void __launch_bounds__(256) naf_dout_kernel(const float* __restrict__ dout, float* __restrict__ deps, int H, int W, int Hp, int Wp,
                                                       size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // (n, y, x) of the padded image
  if (i >= total) return;
  const int px = (int)(i % Wp), py = (int)((i / Wp) % Hp);
  const size_t n = i / ((size_t)Wp * Hp);
  const bool in = py < H && px < W;
#pragma unroll
  for (int c = 0; c < 3; ++c) deps[i * 3 + c] = in ? dout[((n * 3 + c) * H + py) * W + px] : 0.f;
}

// naf_prep_kernel backwards: xin = cat[x - cond, cond], so d x = g[0:3] and d cond = g[3:6] - g[0:3]; the padding's gradient is
// dropped.  g: padded NHWC [N][Hp][Wp][6]; dx, dcond: NCHW H x W, either may be null.
__global__ void __launch_bounds__(256) naf_unprep_kernel(const float* __restrict__ g, float* __restrict__ dx, float* __restrict__ dcond, int H, int W,
                                                         int Hp, int Wp, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // (n, y, x) of the cropped image
  if (i >= total) return;
  const int px = (int)(i % W), py = (int)((i / W) % H);
  const size_t n = i / ((size_t)W * H);
  const float* gp = g + ((n * Hp + py) * Wp + px) * 6;
  const size_t HW = (size_t)H * W, base = n * 3 * HW + (size_t)py * W + px;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = gp[c];
    if (dx) dx[base + c * HW] = a;
    if (dcond) dcond[base + c * HW] = __fsub_rn(gp[3 + c], a);
  }
}

// every scalar is formed on the host in double, as Python forms it, and rounded once (torch hands its kernels such scalars)
struct OptArgs { float lr, b1, b2, omb1, omb2, decay, eps, wd, step_size, bc2_sqrt; int kind; };

// kind 0 Adam (torch's single-tensor path, weight decay as an L2 term of the gradient), 1 AdamW (decoupled), 2 Lion
__global__ void __launch_bounds__(256) naf_optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        OptArgs o, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float w = p[i], gr = g[i], mm = m[i];
  if (o.kind == 2) {
    w = __fmul_rn(w, o.decay);
    const float u = __fadd_rn(__fmul_rn(mm, o.b1), __fmul_rn(gr, o.omb1));
    const float sg = u > 0.f ? 1.f : u < 0.f ? -1.f : 0.f;
    p[i] = __fadd_rn(w, __fmul_rn(-o.lr, sg));
    m[i] = __fadd_rn(__fmul_rn(mm, o.b2), __fmul_rn(o.omb2, gr));
    return;
  }
  if (o.kind == 1) w = __fmul_rn(w, o.decay);
  else if (o.wd != 0.f) gr = __fadd_rn(gr, __fmul_rn(o.wd, w));
  mm = __fadd_rn(mm, __fmul_rn(o.omb1, __fsub_rn(gr, mm)));                                  // exp_avg.lerp_(grad, 1 - beta1)
  const float vv = __fadd_rn(__fmul_rn(v[i], o.b2), __fmul_rn(__fmul_rn(o.omb2, gr), gr));   // mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vv), o.bc2_sqrt), o.eps);
  p[i] = __fadd_rn(w, __fmul_rn(-o.step_size, __fdiv_rn(mm, denom)));
  m[i] = mm;
  v[i] = vv;
}

// every device form again from the master: arena[i] = master[map[i]] where the element holds a weight
__global__ void __launch_bounds__(256) naf_repack_kernel(float* __restrict__ arena, const float* __restrict__ master, const int* __restrict__ map, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int s = map[i];
  if (s >= 0) arena[i] = master[s];
}

// The f16 forms again from the re-packed arena, on the device (f16 training storage: the forward after a step reads the hi planes).
// split_weights' arithmetic per GEMM, bit for bit: the maximum of min(|w|, 65504) over the pack (two passes, WQ_SLICES workgroups per GEMM), e = min(12, floor(log2(32768 / max)))
// from the maximum's exponent and mantissa bits (32768 / max is a power of two exactly when the mantissa is zero), hi = f16(w 2^e),
// lo = f16(w 2^e - hi) in fragment order.  A maximum has no order to keep.
struct WqDesc {
  unsigned long long woff, hoff;   // the pack's first float in the arena, the GEMM's first fragment in d_wq
  unsigned h0;                     // the hi fragments before this GEMM's (a multiple of 256)
  int Kp, Cp, nk;
};

constexpr int WQ_SLICES = 64;   // workgroups per GEMM of the maximum's first pass

// max of min(|w|, 65504) over slice blockIdx.y of GEMM blockIdx.x's pack: part[gemm][slice]
__global__ void __launch_bounds__(256) naf_wq_max_kernel(const float* __restrict__ arena, const WqDesc* __restrict__ desc, float* __restrict__ part) {
  __shared__ float red[256];
  const WqDesc g = desc[blockIdx.x];
  const float* w = arena + g.woff;
  const size_t total = (size_t)g.Kp * g.Cp;
  float amax = 0.f;
  for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < total; i += (size_t)WQ_SLICES * 256) {
    float v = fabsf(w[i]);
    v = F16_MAX < v ? F16_MAX : v;   // std::min / std::max of the host, NaN for NaN
    amax = amax < v ? v : amax;
  }
  red[threadIdx.x] = amax;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] < red[threadIdx.x + o] ? red[threadIdx.x + o] : red[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(size_t)blockIdx.x * WQ_SLICES + blockIdx.y] = red[0];
}

// the slices' maxima -> e and 2^-e of GEMM blockIdx.x; one wave
__global__ void __launch_bounds__(WQ_SLICES) naf_wq_scale_kernel(const float* __restrict__ part, float* __restrict__ hinv, int* __restrict__ hexp) {
  float amax = part[(size_t)blockIdx.x * WQ_SLICES + threadIdx.x];
#pragma unroll
  for (int o = WQ_SLICES / 2; o; o >>= 1) {
    const float other = __shfl_xor(amax, o, WQ_SLICES);
    amax = amax < other ? other : amax;
  }
  if (threadIdx.x == 0) {
    int e = 12;   // max <= 8: 32768 / max >= 2^12
    if (amax > 8.f) {
      const unsigned bits = __float_as_uint(amax);
      e = 15 - ((int)(bits >> 23) - 127) - ((bits & 0x7fffffu) ? 1 : 0);
    }
    hexp[blockIdx.x] = e;
    hinv[blockIdx.x] = __uint_as_float((unsigned)(127 - e) << 23);
  }
}

// one thread per hi fragment (and its lo twin, 64 further): blocks do not straddle GEMMs
__global__ void __launch_bounds__(256) naf_wq_pack_kernel(const float* __restrict__ arena, const WqDesc* __restrict__ desc, int ngemms,
                                                          const int* __restrict__ hexp, uint4* __restrict__ wq, unsigned total) {
  const unsigned gi = blockIdx.x * 256 + threadIdx.x;
  if (gi >= total) return;
  int lo = 0, hi = ngemms - 1;   // the last GEMM whose h0 <= gi
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].h0 <= gi) lo = mid;
    else hi = mid - 1;
  }
  const WqDesc g = desc[lo];
  const float scale = __uint_as_float((unsigned)(127 + hexp[lo]) << 23);
  const unsigned idx = gi - g.h0;
  const int l = idx & 63, s = (idx >> 6) & 1, nb = (idx >> 7) & 1;
  const unsigned rest = idx >> 8;
  const int kc = (int)(rest % (unsigned)g.nk), cot = (int)(rest / (unsigned)g.nk);
  const int col = cot * BN + nb * 32 + (l & 31);
  const float* w = arena + g.woff;
  naf_h8 qh, ql;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = kc * HK + 16 * s + 8 * (l >> 5) + j;
    float v = 0.f;
    if (k < g.Kp) {
      v = w[(size_t)k * g.Cp + col];
      v = v < -F16_MAX ? -F16_MAX : v;
      v = F16_MAX < v ? F16_MAX : v;
      v = __fmul_rn(v, scale);
    }
    qh[j] = (_Float16)v;
    ql[j] = (_Float16)__fsub_rn(v, (float)qh[j]);
  }
  uint4* dst = wq + g.hoff + (size_t)(idx >> 6) * 128 + l;
  dst[0] = __builtin_bit_cast(uint4, qh);
  dst[64] = __builtin_bit_cast(uint4, ql);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

typedef Slots<size_t> BlockSlots;   // workspace offsets

struct TrainPlan {
  int N, H, W, Hp, Wp;
  size_t xin, x0, r1, r, ca, enh, eps, deps, tg, trow, tf, part, losspart;
  size_t gx, gt, gu, g2a, g2b, drows, dtg, small, wgpart, wg_floats;
  std::vector<BlockSlots> blk;
  std::vector<size_t> down, up, dskip;
  size_t bytes;
};

int ilog2(int v) { int l = 0; while ((1 << (l + 1)) <= v) ++l; return l; }

// floats of naf_wgrad_kernel's partial sums for gemm g over M output pixels
size_t wg_need(int K, int cout, int M) {
  return (size_t)((M + WG_CHUNK - 1) / WG_CHUNK) * round_up(K, 64) * round_up(cout, 64);
}

TrainPlan make_train_plan(fdsr_nafnet n, int N, int H, int W) {
  TrainPlan p{};
  const int pad = 1 << n->L, w = n->wd, L = n->L;
  p.N = N; p.H = H; p.W = W;
  p.Hp = round_up(H, pad);
  p.Wp = round_up(W, pad);
  const size_t M0 = (size_t)N * p.Hp * p.Wp;
  size_t off = 0;
  auto buf = [&](size_t floats) { const size_t o = off; off = align_up(off + floats * sizeof(float), 256); return o; };
  // a saved activation: f16 elements under f16 training storage, in a slot of half the bytes
  const size_t esz = mode_of(n, true).h() ? sizeof(_Float16) : sizeof(float);
  auto abuf = [&](size_t elems) { const size_t o = off; off = align_up(off + elems * esz, 256); return o; };
  p.xin = buf(M0 * 6);
  p.x0 = abuf(M0 * w); p.r1 = abuf(M0 * w); p.r = abuf(M0 * w); p.enh = abuf(M0 * w);
  p.ca = buf((size_t)N * w);
  p.eps = buf(M0 * 3); p.deps = buf(M0 * 3);
  p.tg = buf((size_t)N * 2 * w); p.trow = buf((size_t)N * n->R); p.tf = buf(N);
  size_t part = 0;
  for (int l = 0; l <= L; ++l) part = std::max(part, (size_t)nstrips_of((p.Hp >> l) * (p.Wp >> l)) * ((size_t)w << l) * 20);   // 10 [2c] rows of conv2
  p.part = buf((size_t)N * part);
  p.losspart = buf((size_t)N * ((H * W + 1023) / 1024));
  p.gx = buf(M0 * w); p.gt = buf(M0 * w); p.gu = buf(M0 * w); p.g2a = buf(M0 * 2 * w); p.g2b = buf(M0 * 2 * w);
  p.drows = buf((size_t)N * n->R);
  p.dtg = buf((size_t)N * 2 * w);
  p.small = buf((size_t)N * (((size_t)w << L) * 4 + 17 * (size_t)w + 64));
  p.blk.resize(n->blocks.size());
  for (size_t bi = 0; bi < n->blocks.size(); ++bi) {
    const int c = n->blocks[bi].c, l = ilog2(c / w);
    const size_t M = M0 >> (2 * l);
    BlockSlots& s = p.blk[bi];
    s.out = abuf(M * c); s.st1 = buf(M * 2); s.t1 = abuf(M * 2 * c); s.t2 = abuf(M * c); s.sca = buf((size_t)N * c);
    s.y = abuf(M * c); s.st2 = buf(M * 2); s.p4 = abuf(M * 2 * c); s.g4 = abuf(M * c);
  }
  for (int l = 0; l < L; ++l) {
    p.down.push_back(abuf((M0 * w) >> (l + 1)));                // level l + 1
    p.up.push_back(abuf((M0 * w) >> (L - 1 - l)));              // ups[l] lands on level L - 1 - l
    p.dskip.push_back(buf((M0 * w) >> l));
  }
  size_t wg = 0;
  for (const GemmL& g : n->gemms) {
    const int l = g.cin < w ? 0 : ilog2(g.cin / w);
    const size_t M = g.ks == 2 ? M0 >> (2 * (l + 1)) : M0 >> (2 * l);
    wg = std::max(wg, wg_need(g.K() + 1, g.cout, (int)M));
  }
  p.wg_floats = wg;
  p.wgpart = buf(wg);
  p.bytes = off;
  return p;
}

int ensure_train(fdsr_nafnet n) {
  if (!n->d_master) {
    for (float** q : {&n->d_master, &n->d_grad, &n->d_m, &n->d_v}) {
      HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(q), n->P * sizeof(float)));
      HIPCHK(nullptr, hipMemset(*q, 0, n->P * sizeof(float)));
    }
    std::vector<int> map(n->arena_floats, -1);
    IndexSink sink{n, map};
    pack_forms(n, sink);
    HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_map), map.size() * sizeof(int)));
    HIPCHK(nullptr, hipMemcpy(n->d_map, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
    std::vector<int> rm(3 * (size_t)n->R, -1);
    const int K2 = 2 * n->wd;
    for (const BlockL& b : n->blocks)
      for (int r = 0; r < 4 * b.c; ++r) {
        const int gr = b.row_off + r, chunk = r / b.c, ch = r % b.c;
        rm[gr] = (int)(n->poff[b.mlpw] + (size_t)r * K2);
        rm[n->R + gr] = (int)(n->poff[b.mlpb] + r);
        rm[2 * n->R + gr] = chunk == 1 ? (int)(n->poff[b.g1] + ch) : chunk == 3 ? (int)(n->poff[b.g2] + ch) : -1;
      }
    HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_rowmap), rm.size() * sizeof(int)));
    HIPCHK(nullptr, hipMemcpy(n->d_rowmap, rm.data(), rm.size() * sizeof(int), hipMemcpyHostToDevice));
    // the device rebuild of the f16 forms: each GEMM's place; its exponent e and the maximum's partial results after the table
    std::vector<WqDesc> desc;
    for (const GemmL& g : n->gemms) desc.push_back({g.woff, g.hoff, (unsigned)(g.hoff / 2), g.Kpad(), g.CoutPad(), g.K32() / HK});
    HIPCHK(nullptr, hipMalloc(&n->d_hdesc, desc.size() * (sizeof(WqDesc) + sizeof(int) + WQ_SLICES * sizeof(float))));
    HIPCHK(nullptr, hipMemcpy(n->d_hdesc, desc.data(), desc.size() * sizeof(WqDesc), hipMemcpyHostToDevice));
  }
  if (!n->master_valid) {
    HIPCHK(nullptr, hipDeviceSynchronize());
    for (size_t i = 0; i < n->wts.size(); ++i)
      HIPCHK(nullptr, hipMemcpy(n->d_master + n->poff[i], n->wts[i].host.data(), n->wts[i].host.size() * sizeof(float), hipMemcpyHostToDevice));
    n->master_valid = true;
  }
  return FDSR_OK;
}

// after a re-pack under f16 training storage: the f16 forms and their scales follow the arena, stream-ordered, no host round trip
int rebuild_wq(fdsr_nafnet n, hipStream_t st) {
  if (!mode_of(n, true).h()) return FDSR_OK;
  const WqDesc* desc = static_cast<const WqDesc*>(n->d_hdesc);
  int* hexp = reinterpret_cast<int*>(static_cast<char*>(n->d_hdesc) + n->gemms.size() * sizeof(WqDesc));
  const unsigned total = (unsigned)(n->hfrags / 2);
  float* part = reinterpret_cast<float*>(hexp + n->gemms.size());   // [gemms][WQ_SLICES]
  hipLaunchKernelGGL(naf_wq_max_kernel, dim3((unsigned)n->gemms.size(), WQ_SLICES), dim3(256), 0, st, n->d_arena, desc, part);
  HIPCHK(nullptr, hipGetLastError());
  hipLaunchKernelGGL(naf_wq_scale_kernel, dim3((unsigned)n->gemms.size()), dim3(WQ_SLICES), 0, st, part, n->d_hinv, hexp);
  HIPCHK(nullptr, hipGetLastError());
  hipLaunchKernelGGL(naf_wq_pack_kernel, dim3(total / 256), dim3(256), 0, st, n->d_arena, desc, (int)n->gemms.size(), hexp, n->d_wq, total);
  HIPCHK(nullptr, hipGetLastError());
  return FDSR_OK;
}

// The master changed on the device (an optimizer step, fdsr_nafnet_set_weights_flat): every device form follows it, stream-ordered;
// the host copies and the row table are behind, and a captured graph holds nothing to keep.
int master_moved(fdsr_nafnet n, hipStream_t st) {
  hipLaunchKernelGGL(naf_repack_kernel, dim3(Run::nb(n->arena_floats)), dim3(256), 0, st, n->d_arena, n->d_master, n->d_map, n->arena_floats);
  HIPCHK(nullptr, hipGetLastError());
  const int rc = rebuild_wq(n, st);
  if (rc) return rc;
  n->host_stale = true; n->table_valid = false;
  drop_graph(n);
  return FDSR_OK;
}

size_t train_plan_bytes(fdsr_nafnet n, int N, int H, int W) { return make_train_plan(n, N, H, W).bytes; }

// the forward walk's table for training: every tensor in its own slot, and every chain of blocks wanted where it ends (no copies).
// The saved activations (make_train_plan's abuf slots) are f16 under h.
NetDst train_dst(fdsr_nafnet n, const TrainPlan& tp, char* ws, bool h) {
  auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
  auto A = [&](size_t off) { return Act{F(off), h}; };
  NetDst d{};
  d.N = tp.N; d.H = tp.H; d.W = tp.W; d.Hp = tp.Hp; d.Wp = tp.Wp;
  d.xin = F(tp.xin); d.intro = A(tp.x0); d.r1 = A(tp.r1); d.r = A(tp.r); d.ca = F(tp.ca); d.enh = A(tp.enh); d.eps = F(tp.eps);
  d.part = F(tp.part); d.tg = F(tp.tg); d.trow = F(tp.trow);
  for (const BlockSlots& s : tp.blk)
    d.blk.push_back({A(s.out), F(s.st1), A(s.t1), A(s.t2), F(s.sca), A(s.y), F(s.st2), A(s.p4), A(s.g4)});
  auto end = [&](const std::vector<int>& list, Act first) { return list.empty() ? first : d.blk[list.back()].out; };
  for (int i = 0; i < n->L; ++i) {
    d.down[i] = A(tp.down[i]);
    d.up[i] = A(tp.up[i]);
    d.skip[i] = end(n->enc[i], i ? d.down[i - 1] : d.enh);
    d.dec[i] = end(n->dec[i], d.up[i]);
  }
  d.mid = end(n->mid, d.down[n->L - 1]);
  return d;
}

typedef void (*WgradFn)(WgArgs);
template <int XS> WgradFn wgrad_fn(int pro) {   // XS: the stored type of x; dy is fp32
  return pro == PRO_LN    ? naf_wgrad_kernel<PRO_LN, XS, ACT_F32>
         : pro == PRO_MUL ? naf_wgrad_kernel<PRO_MUL, XS, ACT_F32>
                          : naf_wgrad_kernel<PRO_NONE, XS, ACT_F32>;
}

// Run's forward walk over train_dst, then the backward over what it left there
struct TrainRun : Run {
  TrainPlan tp;
  char* ws;

  float* F(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  float* G(int wi) const { return n->d_grad + n->poff[wi]; }

  // the input of block j of a list whose first block reads `first`
  Act chain_in(const std::vector<int>& list, size_t j, Act first) const { return j == 0 ? first : d.blk[list[j - 1]].out; }

  // ---- backward launchers ----
  // A saved activation is f16 under f16 training storage: SEL picks the kernel instance for the stored type of the operand that is
  // one.  Gradients are fp32 always (plain float*: Run::copy moves them as such).
#define NAF_SEL1(K, act) ((act).h ? K<ACT_F16> : K<ACT_F32>)
  // An input gradient: gemms[gi]'s transposed pack as a convolution of its own.  Gradients are fp32 and the transposed packs have no
  // f16 form, so this is the exact kernel in every mode.
  void tgemm(int gi, float* g, float* out, int h, int w, Pro pro = {}, Epi epi = {}) { gemm_l(n->tgemms[gi], FORM_F32, g, out, h, w, pro, epi); }

  // weight (and bias) gradient of gemm gi: x its forward input (Hin x Win) under the forward's prologue, dy [M][cout]
  void wgrad(int gi, Act x, float* dy, int Hin, int Win, Pro pro = {}, const float* colmul = nullptr) {
    const GemmL& g = n->gemms[gi];
    wgrad_l(g, x, dy, Hin, Win, pro, colmul, 0, G(g.w), g.b >= 0 ? G(g.b) : nullptr);
  }

  // g: the convolution in the kernel's terms; x, dy: its two operands, either of which may be a saved activation (dy: ups only, whose
  // g is the transposed convolution, operands exchanged, mode 1); gw, gb: where the finished sums go
  void wgrad_l(const GemmL& g, Act x, Act dy, int Hin, int Win, Pro pro, const float* colmul, int mode, float* gw, float* gb) {
    WgArgs a{};
    a.x = x; a.dy = dy; a.stats = pro.stats; a.pmul = pro.pmul; a.padd = pro.padd; a.colmul = colmul; a.part = F(tp.wgpart);
    a.N = tp.N; a.Hin = Hin; a.Win = Win; a.Cin = g.cin;
    a.Hout = (Hin + 2 * g.p - g.ks) / g.s + 1;
    a.Wout = (Win + 2 * g.p - g.ks) / g.s + 1;
    a.Cout = g.cout; a.KW = g.ks; a.S = g.s; a.P = g.p; a.K = g.K(); a.Keff = gb ? a.K + 1 : a.K; a.ldy = g.cout; a.pstride = pro.pstride;
    const int M = a.N * a.Hout * a.Wout, nz = (M + WG_CHUNK - 1) / WG_CHUNK;
    const dim3 grid((unsigned)((a.Keff + 63) / 64), (unsigned)((a.Cout + 63) / 64), (unsigned)nz);
    if ((size_t)nz * grid.x * 64 * grid.y * 64 > tp.wg_floats) {
      if (err == FDSR_OK) err = fail(nullptr, FDSR_E_WORKSPACE, "fdsr_nafnet: weight-gradient scratch too small");
      return;
    }
    // dy.h is ups' (no prologue): the gathered gradient is A, the saved input is "dy"
    WgradFn k = x.h ? wgrad_fn<ACT_F16>(pro.kind) : wgrad_fn<ACT_F32>(pro.kind);
    if (dy.h) k = naf_wgrad_kernel<PRO_NONE, ACT_F32, ACT_F16>;
    launch(k, grid, dim3(256), 0, a);
    launch(naf_wgrad_finish_kernel, dim3(nb((size_t)a.Keff * a.Cout)), dim3(256), 0, a.part, nz, (int)grid.x * 64, (int)grid.y * 64, a.Keff, a.K,
           a.Cout, a.Cin, g.ks * g.ks, mode, gw, gb);
  }

  // per-channel sums over pixels: dst[g][ch], groups = N (per image, rows dstride apart) or 1 (everything); a or b may be a saved activation
  void dot(Act a, Act b, const float* stats, int mode, int HW, int c, float* dst, bool per_image, int dstride, float scale = 1.f) {
    const int ns = nstrips_of(HW);
    launch(a.h ? naf_dot_kernel<ACT_F16, ACT_F32> : b.h ? naf_dot_kernel<ACT_F32, ACT_F16> : naf_dot_kernel<ACT_F32, ACT_F32>,
           dim3((unsigned)ns, (unsigned)((c + 63) / 64), (unsigned)tp.N), dim3(256), 0, a, b, stats, d.part, HW, c, ns, mode);
    const int groups = per_image ? tp.N : 1, Gn = per_image ? ns : tp.N * ns;
    launch(naf_reduce_kernel, dim3(nb((size_t)groups * c)), dim3(256), 0, d.part, dst, groups, Gn, c, scale, dstride);
  }

  // LayerNorm + FiLM backward: g += d x; the image's d (folded scale) and d shift rows into drows
  void ln_bwd(Act x, float* dy, const float* stats, const float* mulrow, float* g, int HW, int c, float* dmul, float* dadd) {
    const int M = tp.N * HW;
    dot(dy, x, stats, 2, HW, c, dmul, true, n->R);
    dot(dy, nullptr, nullptr, 0, HW, c, dadd, true, n->R);
    launch(NAF_SEL1(naf_ln_bwd_kernel, x), dim3((unsigned)((M + 15) / 16)), dim3(256), 0, x, dy, stats, mulrow, rstride, g, M, HW, c);
  }

  // g: d out on entry, d inp on return (in place); cur: the block's input
  void block_bwd(int bi, Act cur, float* g, int h, int w) {
    const BlockL& b = n->blocks[bi];
    const BlockDst& s = d.blk[bi];
    const int c = b.c, HW = h * w, M = tp.N * HW, ns = nstrips_of(HW);
    const size_t tot = (size_t)M * c;
    const float* rw = rows + b.row_off;
    float *gt = F(tp.gt), *g2a = F(tp.g2a), *g2b = F(tp.g2b), *dr = F(tp.drows) + b.row_off;
    float* sm = F(tp.small);
    float *ds = sm, *pooled = sm + (size_t)tp.N * c, *dpool = sm + 2 * (size_t)tp.N * c;
    // out = y + conv5(g4) gamma.  For d gamma (d beta below) conv5's (conv3's) output is formed again into the fp32 gt by the forward's
    // own kernel and operands: under f16 storage the very value the forward scaled
    gemm(b.conv5, s.g4, gt, h, w);
    dot(g, gt, nullptr, 1, HW, c, G(b.gamma), false, 0);
    wgrad(b.conv5, s.g4, g, h, w, {}, P(b.off_gamma));
    tgemm(b.conv5, g, gt, h, w, scaled(P(b.off_gamma), 0));
    launch(NAF_SEL1(naf_gate_bwd_kernel, s.p4), dim3(nb(tot)), dim3(256), 0, gt, s.p4, g2a, c, tot);
    wgrad(b.conv4, s.y, g2a, h, w, ln(s.st2, rw + 3 * c, rw + 2 * c, rstride));
    tgemm(b.conv4, g2a, gt, h, w);
    ln_bwd(s.y, gt, s.st2, rw + 3 * c, g, HW, c, dr + 3 * c, dr + 2 * c);
    // y = inp + conv3(t2 sca) beta
    gemm(b.conv3, s.t2, gt, h, w, scaled(s.sca, c));
    dot(g, gt, nullptr, 1, HW, c, G(b.beta), false, 0);
    wgrad(b.conv3, s.t2, g, h, w, scaled(s.sca, c), P(b.off_beta));
    tgemm(b.conv3, g, gt, h, w, scaled(P(b.off_beta), 0));
    dot(gt, s.t2, nullptr, 1, HW, c, ds, true, c);
    dot(s.t2, nullptr, nullptr, 0, HW, c, pooled, true, c, 1.f / (float)HW);
    launch(naf_sca_bwd_w_kernel, dim3(nb((size_t)c * c)), dim3(256), 0, ds, pooled, G(b.scaw), G(b.scab), tp.N, c);
    launch(naf_sca_bwd_x_kernel, dim3(nb((size_t)tp.N * c)), dim3(256), 0, ds, P(b.off_scaw), dpool, tp.N, c, 1.f / (float)HW);
    launch(NAF_SEL1(naf_dwgate_bwd_kernel, s.t1), dim3(nb(tot)), dim3(256), 0, s.t1, P(b.off_dww), P(b.off_dwb), gt, s.sca, dpool, g2a, h, w, c, tot);
    launch(NAF_SEL1(naf_dw_bwd_kernel, s.t1), dim3((unsigned)ns, (unsigned)((2 * c + 63) / 64), (unsigned)tp.N), dim3(256), 0, s.t1, P(b.off_dww), g2a, g2b,
           d.part, h, w, 2 * c, ns);
    launch(naf_dw_finish_kernel, dim3(nb((size_t)20 * c)), dim3(256), 0, d.part, tp.N * ns, 2 * c, G(b.dww), G(b.dwb));
    wgrad(b.conv1, cur, g2b, h, w, ln(s.st1, rw + c, rw, rstride));
    tgemm(b.conv1, g2b, gt, h, w);
    ln_bwd(cur, gt, s.st1, rw + c, g, HW, c, dr + c, dr);
  }

  void chain_bwd(const std::vector<int>& list, Act first, float* g, int h, int w) {
    for (size_t j = list.size(); j-- > 0;) block_bwd(list[j], chain_in(list, j, first), g, h, w);
  }

  void net_bwd() {
    const int wd = n->wd, L = n->L;
    int h = tp.Hp, w = tp.Wp, c = wd;
    float *g = F(tp.gx), *gt = F(tp.gt), *gu = F(tp.gu);
    wgrad(n->g_ending, d.dec[L - 1], F(tp.deps), h, w);
    tgemm(n->g_ending, F(tp.deps), g, h, w);
    for (int i = L - 1; i >= 0; --i) {
      chain_bwd(n->dec[i], d.up[i], g, h, w);
      // ups[i]: g is d (shuffle(conv(x)) + skip).  The skip's share is g itself; the convolution's is a 2x2 stride-2 gather of g.
      float* dskip = F(tp.dskip[L - 1 - i]);
      copy(dskip, g, (size_t)tp.N * h * w * c);
      // operands exchanged: the gathered gradient is A, ups[i]'s forward input is "dy"
      wgrad_l(n->tgemms[n->ups[i]], dskip, i ? d.dec[i - 1] : d.mid, h, w, {}, nullptr, 1, G(n->gemms[n->ups[i]].w), nullptr);
      tgemm(n->ups[i], dskip, g, h, w);
      h /= 2; w /= 2; c *= 2;
    }
    chain_bwd(n->mid, d.down[L - 1], g, h, w);
    for (int i = L - 1; i >= 0; --i) {
      // downs[i]: g is d out at level i + 1
      wgrad(n->downs[i], d.skip[i], g, 2 * h, 2 * w);
      tgemm(n->downs[i], g, gt, h, w, {}, shuffled(F(tp.dskip[i])));
      h *= 2; w *= 2; c /= 2;
      copy(g, gt, (size_t)tp.N * h * w * c);
      chain_bwd(n->enc[i], i ? d.down[i - 1] : d.enh, g, h, w);
    }
    // enh = x0 + (r a + x0), a = CA(mean r)
    const int HW = h * w, ns = nstrips_of(HW), cs = wd / 16;
    const size_t tot = (size_t)tp.N * HW * wd;
    float* sm = F(tp.small);
    float *da = sm, *dz2 = sm + (size_t)tp.N * wd, *pooled = sm + 2 * (size_t)tp.N * wd, *dpool = sm + 3 * (size_t)tp.N * wd,
          *dz1 = sm + 4 * (size_t)tp.N * wd, *hid = dz1 + (size_t)tp.N * cs;
    dot(g, d.r, nullptr, 1, HW, wd, da, true, wd);
    chansum(d.r, HW, ns);
    launch(naf_ca_bwd_kernel, dim3((unsigned)tp.N), dim3(256), (3 * wd + 256 + 2 * cs) * sizeof(float), d.part, ns, HW, P(n->off_ca1w),
           P(n->off_ca1b), P(n->off_ca2w), d.ca, da, dz2, dz1, hid, pooled, dpool, wd, cs);
    launch(naf_linear_w_kernel, dim3(nb((size_t)wd * cs)), dim3(256), 0, dz2, hid, G(n->ca2w), G(n->ca2b), tp.N, wd, cs);
    launch(naf_linear_w_kernel, dim3(nb((size_t)wd * cs)), dim3(256), 0, dz1, pooled, G(n->ca1w), G(n->ca1b), tp.N, cs, wd);
    launch(naf_scale_add_kernel, dim3(nb(tot)), dim3(256), 0, g, d.ca, dpool, gt, HW, wd, tot);
    wgrad(n->g_rcab2, d.r1, gt, h, w);
    tgemm(n->g_rcab2, gt, gu, h, w);
    launch(NAF_SEL1(naf_relu_mask_kernel, d.r1), dim3(nb(tot)), dim3(256), 0, gu, d.r1, tot);
    wgrad(n->g_rcab0, d.intro, gu, h, w);
    tgemm(n->g_rcab0, gu, gt, h, w);
    launch(naf_twice_plus_kernel, dim3(nb(tot)), dim3(256), 0, g, gt, tot);
    wgrad(n->g_intro, d.xin, g, h, w);
  }

  // past wgrad(g_intro): d xin through intro's transposed pack, then naf_prep_kernel backwards.  net_bwd() left d intro in gx; gt
  // is free from there on and holds d xin [N][Hp][Wp][6].
  void input_bwd(float* dx, float* dcond) {
    tgemm(n->g_intro, F(tp.gx), F(tp.gt), tp.Hp, tp.Wp);
    const size_t total = (size_t)tp.N * tp.H * tp.W;
    launch(naf_unprep_kernel, dim3(nb(total)), dim3(256), 0, F(tp.gt), dx, dcond, tp.H, tp.W, tp.Hp, tp.Wp, total);
  }

  // the rows back through every block's Linear, SimpleGate and time_mlp
  void time_bwd() {
    const int wd = n->wd, K2 = 2 * wd, R = n->R, N = tp.N;
    launch(naf_rows_bwd_kernel, dim3(nb(R)), dim3(256), 0, d.tg, P(n->off_rowsw), P(n->off_rowsb), P(n->off_rowsmul), n->d_rowmap, F(tp.drows),
           n->d_grad, N, K2, R);
    launch(naf_dtg_kernel, dim3((unsigned)K2, (unsigned)N), dim3(256), 0, F(tp.drows), P(n->off_rowsw), F(tp.dtg), K2, R);
    float* sm = F(tp.small);
    float *dh2 = sm, *g1 = sm + (size_t)N * 4 * wd, *dh1 = sm + (size_t)N * 8 * wd, *emb = sm + (size_t)N * 16 * wd;
    launch(naf_time_bwd_kernel, dim3((unsigned)N), dim3(256), 21 * wd * sizeof(float), F(tp.tf), P(n->off_freq), P(n->off_t1w), P(n->off_t1b),
           P(n->off_t2w), P(n->off_t2b), F(tp.dtg), dh2, g1, dh1, emb, wd);
    launch(naf_linear_w_kernel, dim3(nb((size_t)16 * wd * wd)), dim3(256), 0, dh2, g1, G(n->t2w), G(n->t2b), N, 4 * wd, 4 * wd);
    launch(naf_linear_w_kernel, dim3(nb((size_t)8 * wd * wd)), dim3(256), 0, dh1, emb, G(n->t1w), G(n->t1b), N, 8 * wd, wd);
  }
#undef NAF_SEL1
};

// what train_grads, forward_train and backward check alike; the messages are train_grads'
int check_train_call(fdsr_nafnet n, const char* fn, int batch, int height, int width, void* workspace, size_t workspace_bytes) {
  const int rc = check_args(n, fn, batch, height, width, workspace, workspace_bytes, train_plan_bytes);
  return rc ? rc : refuse_training(n, fn, true);
}

// the TrainRun of a checked call: its plan, the walk's table over the workspace, training's mode
TrainRun train_run(fdsr_nafnet n, int batch, int height, int width, void* workspace, void* hip_stream) {
  char* ws = static_cast<char*>(workspace);
  const TrainPlan tp = make_train_plan(n, batch, height, width);
  const Mode m = mode_of(n, true);
  return TrainRun{{n, m, train_dst(n, tp, ws, m.h()), reinterpret_cast<hipStream_t>(hip_stream), nullptr, n->R}, tp, ws};
}

int find_weight(fdsr_nafnet n, const char* fn, const char* key) {
  if (!n || !key) return fail(nullptr, FDSR_E_INVALID, "%s: null argument", fn);
  const auto it = n->key2w.find(key);
  if (it == n->key2w.end()) return fail(nullptr, FDSR_E_KEY, "%s: unknown tensor '%s'", fn, key);
  return it->second;
}

}  // namespace

extern "C" {

int fdsr_nafnet_set_thetas_cumsum(fdsr_nafnet n, int T, const float* thetas_cumsum) {
  if (!n || !thetas_cumsum || T < 1) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_set_thetas_cumsum: bad arguments (T %d)", T);
  if (n->T != T) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_set_thetas_cumsum: T %d is not the schedule's (fdsr_nafnet_set_sde first)", T);
  HIPCHK(nullptr, hipDeviceSynchronize());
  if (n->d_cum) { (void)hipFree(n->d_cum); n->d_cum = nullptr; }
  HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&n->d_cum), (size_t)(T + 1) * sizeof(float)));
  HIPCHK(nullptr, hipMemcpy(n->d_cum, thetas_cumsum, (size_t)(T + 1) * sizeof(float), hipMemcpyHostToDevice));
  n->cum_T = T;
  return FDSR_OK;
}

int fdsr_nafnet_train_workspace_bytes(fdsr_nafnet n, int batch, int height, int width, size_t* bytes) {
  if (!n || !bytes || batch < 1 || height < 1 || width < 1)
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_train_workspace_bytes: bad arguments (B %d, %dx%d)", batch, height, width);
  *bytes = train_plan_bytes(n, batch, height, width);
  return FDSR_OK;
}

int fdsr_nafnet_train_grads(fdsr_nafnet n, const float* state_nchw, const float* cond_nchw, const float* gt_nchw, const int32_t* timesteps_dev,
                            int loss_type, float weight, float* loss_out_dev, int batch, int height, int width, void* workspace,
                            size_t workspace_bytes, void* hip_stream) {
  const char* fn = "fdsr_nafnet_train_grads";
  if (!n || !state_nchw || !cond_nchw || !gt_nchw || !timesteps_dev || !loss_out_dev || !workspace || batch < 1 || height < 1 || width < 1)
    return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, batch, height, width);
  if (loss_type & FDSR_NAFNET_LOSS_WEIGHTED) return fail(nullptr, FDSR_E_INVALID, "%s: is_weighted is not supported (the reference passes no weights)", fn);
  if (loss_type != FDSR_NAFNET_LOSS_L1 && loss_type != FDSR_NAFNET_LOSS_L2) return fail(nullptr, FDSR_E_INVALID, "%s: loss_type %d (l1 = 0, l2 = 1)", fn, loss_type);
  int rc = check_train_call(n, fn, batch, height, width, workspace, workspace_bytes);
  if (rc) return rc;
  if (n->T < 1 || n->cum_T != n->T) return fail(nullptr, FDSR_E_STATE, "%s: no schedule (fdsr_nafnet_set_sde, fdsr_nafnet_set_thetas_cumsum)", fn);
  if ((rc = ensure_train(n))) return rc;
  kill_ticket(n, fn);
  TrainRun t = train_run(n, batch, height, width, workspace, hip_stream);
  const TrainPlan& tp = t.tp;
  HIPCHK(nullptr, hipMemsetAsync(n->d_grad, 0, n->P * sizeof(float), t.st));
  HIPCHK(nullptr, hipMemsetAsync(t.F(tp.deps), 0, (size_t)batch * tp.Hp * tp.Wp * 3 * sizeof(float), t.st));
  t.launch(naf_i2f_kernel, dim3(Run::nb(batch)), dim3(256), 0, timesteps_dev, t.F(tp.tf), batch);
  t.forward(state_nchw, cond_nchw, t.F(tp.tf));
  {
    LossTables tb{n->d_sde, n->d_sde + (n->T + 1), n->d_sde + 2 * (n->T + 1), n->d_cum, n->dt, n->T};
    const int HW = height * width, nblk = (HW + 1023) / 1024;
    const float gscale = weight / ((float)batch * 3.f * (float)HW);
    t.launch(naf_loss_kernel, dim3((unsigned)nblk, (unsigned)batch), dim3(256), 0, t.d.eps, state_nchw, cond_nchw, gt_nchw, timesteps_dev, tb,
             loss_type == FDSR_NAFNET_LOSS_L2 ? 1 : 0, gscale, t.F(tp.deps), t.F(tp.losspart), height, width, tp.Hp, tp.Wp);
    t.launch(naf_loss_finish_kernel, dim3(1), dim3(64), 0, t.F(tp.losspart), nblk, batch, 1.f / (3.f * (float)HW), weight, loss_out_dev);
  }
  t.net_bwd();
  t.time_bwd();
  return t.err;
}

int fdsr_nafnet_forward_train(fdsr_nafnet n, const float* x_nchw, const float* cond_nchw, const float* time_dev, float* out_nchw, int batch,
                              int height, int width, void* workspace, size_t workspace_bytes, int64_t* ticket, void* hip_stream) {
  const char* fn = "fdsr_nafnet_forward_train";
  if (!n || !x_nchw || !cond_nchw || !time_dev || !out_nchw || !ticket || !workspace || batch < 1 || height < 1 || width < 1)
    return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, batch, height, width);
  int rc = check_train_call(n, fn, batch, height, width, workspace, workspace_bytes);
  if (rc) return rc;
  if ((rc = ensure_train(n))) return rc;
  kill_ticket(n, "a second fdsr_nafnet_forward_train");
  TrainRun t = train_run(n, batch, height, width, workspace, hip_stream);
  HIPCHK(nullptr, hipMemcpyAsync(t.F(t.tp.tf), time_dev, (size_t)batch * sizeof(float), hipMemcpyDeviceToDevice, t.st));   // time_bwd reads it
  t.forward(x_nchw, cond_nchw, t.F(t.tp.tf));
  t.tail(0, out_nchw, nullptr, nullptr, nullptr, 0, 0);
  if (t.err) return t.err;
  n->ticket.live = ++n->ticket.next;
  n->ticket.N = batch; n->ticket.H = height; n->ticket.W = width; n->ticket.ws = workspace;
  *ticket = n->ticket.live;
  return FDSR_OK;
}

int fdsr_nafnet_backward(fdsr_nafnet n, int64_t ticket, const float* d_out_nchw, float* d_x_nchw, float* d_cond_nchw, int batch, int height,
                         int width, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* fn = "fdsr_nafnet_backward";
  if (!n || !d_out_nchw || !workspace || batch < 1 || height < 1 || width < 1)
    return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments (B %d, %dx%d)", fn, batch, height, width);
  if (ticket < 1 || ticket != n->ticket.live)
    return fail(nullptr, FDSR_E_STATE, "%s: ticket %lld is stale: %s came after its forward, and the activations it kept are not there any more", fn,
                (long long)ticket, n->ticket.live ? "a second fdsr_nafnet_forward_train" : n->ticket.killer);
  if (batch != n->ticket.N || height != n->ticket.H || width != n->ticket.W || workspace != n->ticket.ws)
    return fail(nullptr, FDSR_E_INVALID, "%s: B %d at %dx%d and the workspace must be those of the ticket's forward (B %d at %dx%d)", fn, batch, height,
                width, n->ticket.N, n->ticket.H, n->ticket.W);
  int rc = check_train_call(n, fn, batch, height, width, workspace, workspace_bytes);
  if (rc) return rc;
  kill_ticket(n, "an earlier fdsr_nafnet_backward (it consumes the ticket)");
  TrainRun t = train_run(n, batch, height, width, workspace, hip_stream);
  const TrainPlan& tp = t.tp;
  t.rows = t.d.trow;   // the forward's
  HIPCHK(nullptr, hipMemsetAsync(n->d_grad, 0, n->P * sizeof(float), t.st));
  const size_t total = (size_t)batch * tp.Hp * tp.Wp;
  t.launch(naf_dout_kernel, dim3(Run::nb(total)), dim3(256), 0, d_out_nchw, t.F(tp.deps), height, width, tp.Hp, tp.Wp, total);
  t.net_bwd();
  if (d_x_nchw || d_cond_nchw) t.input_bwd(d_x_nchw, d_cond_nchw);
  t.time_bwd();
  return t.err;
}

int fdsr_nafnet_copy_grads(fdsr_nafnet n, float* dst_dev, size_t count, void* hip_stream) {
  if (!n || !dst_dev) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_copy_grads: null argument");
  if (!n->d_grad) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_copy_grads: no gradients yet (fdsr_nafnet_train_grads, fdsr_nafnet_backward)");
  if (count != n->P) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_copy_grads: count %zu is not the %zu floats of the flat gradient", count, n->P);
  HIPCHK(nullptr, hipMemcpyAsync(dst_dev, n->d_grad, n->P * sizeof(float), hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(hip_stream)));
  return FDSR_OK;
}

int fdsr_nafnet_set_weights_flat(fdsr_nafnet n, const float* src_dev, size_t count, void* hip_stream) {
  const char* fn = "fdsr_nafnet_set_weights_flat";
  if (!n || !src_dev) return fail(nullptr, FDSR_E_INVALID, "%s: null argument", fn);
  if (count != n->P) return fail(nullptr, FDSR_E_INVALID, "%s: count %zu is not the %zu floats of all tensors", fn, count, n->P);
  int rc = refuse_training(n, fn, false);
  if (rc) return rc;
  if ((rc = finalize(n))) return rc;   // the first upload is the host's (fdsr_nafnet_load_weight): it sets the constants of the arena
  if ((rc = ensure_train(n))) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIPCHK(nullptr, hipMemcpyAsync(n->d_master, src_dev, n->P * sizeof(float), hipMemcpyDeviceToDevice, st));
  if ((rc = master_moved(n, st))) return rc;
  kill_ticket(n, fn);
  return FDSR_OK;
}

int fdsr_nafnet_grad_buffer(fdsr_nafnet n, float** device_ptr, size_t* count) {
  if (!n || !device_ptr || !count) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_grad_buffer: null argument");
  if (!n->d_grad) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_grad_buffer: no gradients yet (fdsr_nafnet_train_grads)");
  *device_ptr = n->d_grad;
  *count = n->P;
  return FDSR_OK;
}

int fdsr_nafnet_read_grad(fdsr_nafnet n, const char* key, float* host_f32) {
  if (!host_f32) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_read_grad: null argument");
  const int wi = find_weight(n, "fdsr_nafnet_read_grad", key);
  if (wi < 0) return wi;
  if (!n->d_grad) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_read_grad: no gradients yet (fdsr_nafnet_train_grads)");
  HIPCHK(nullptr, hipDeviceSynchronize());
  HIPCHK(nullptr, hipMemcpy(host_f32, n->d_grad + n->poff[wi], numel(n->wts[wi].shape) * sizeof(float), hipMemcpyDeviceToHost));
  return FDSR_OK;
}

int fdsr_nafnet_optim_step(fdsr_nafnet n, int kind, double lr, double beta1, double beta2, double eps, double weight_decay, void* hip_stream) {
  if (!n || kind < FDSR_NAFNET_ADAM || kind > FDSR_NAFNET_LION || !(lr >= 0.) || !(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.) ||
      !(eps >= 0.) || !(weight_decay >= 0.))
    return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_optim_step: bad arguments (kind %d)", kind);
  const int rc = refuse_training(n, "fdsr_nafnet_optim_step", false);
  if (rc) return rc;
  if (!n->d_grad || !n->master_valid || n->dirty) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_optim_step: no gradients (fdsr_nafnet_train_grads first)");
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  kill_ticket(n, "fdsr_nafnet_optim_step");
  n->opt_step += 1;
  OptArgs o{};
  o.kind = kind; o.lr = (float)lr; o.b1 = (float)beta1; o.b2 = (float)beta2; o.eps = (float)eps; o.wd = (float)weight_decay;
  o.omb1 = (float)(1.0 - beta1); o.omb2 = (float)(1.0 - beta2); o.decay = (float)(1.0 - lr * weight_decay);
  const double bc1 = 1.0 - std::pow(beta1, (double)n->opt_step), bc2 = 1.0 - std::pow(beta2, (double)n->opt_step);
  o.step_size = (float)(lr / bc1);
  o.bc2_sqrt = (float)std::sqrt(bc2);
  hipLaunchKernelGGL(naf_optim_kernel, dim3(Run::nb(n->P)), dim3(256), 0, st, n->d_master, n->d_grad, n->d_m, n->d_v, o, n->P);
  HIPCHK(nullptr, hipGetLastError());
  return master_moved(n, st);
}

int fdsr_nafnet_read_weight(fdsr_nafnet n, const char* key, float* dst, int dst_on_device, void* hip_stream) {
  if (!dst) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_read_weight: null argument");
  const int wi = find_weight(n, "fdsr_nafnet_read_weight", key);
  if (wi < 0) return wi;
  const WT& w = n->wts[wi];
  if (!w.loaded) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_read_weight: tensor '%s' is missing", key);
  const size_t bytes = numel(w.shape) * sizeof(float);
  if (!n->host_stale) {   // the host copy is current
    if (dst_on_device) HIPCHK(nullptr, hipMemcpyAsync(dst, w.host.data(), bytes, hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(hip_stream)));
    else memcpy(dst, w.host.data(), bytes);
    if (dst_on_device) HIPCHK(nullptr, hipStreamSynchronize(reinterpret_cast<hipStream_t>(hip_stream)));
    return FDSR_OK;
  }
  if (dst_on_device) {
    HIPCHK(nullptr, hipMemcpyAsync(dst, n->d_master + n->poff[wi], bytes, hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(hip_stream)));
  } else {
    HIPCHK(nullptr, hipStreamSynchronize(reinterpret_cast<hipStream_t>(hip_stream)));
    HIPCHK(nullptr, hipMemcpy(dst, n->d_master + n->poff[wi], bytes, hipMemcpyDeviceToHost));
  }
  return FDSR_OK;
}

int fdsr_nafnet_optim_get_state(fdsr_nafnet n, const char* key, float* exp_avg_host, float* exp_avg_sq_host, int64_t* step) {
  const int wi = find_weight(n, "fdsr_nafnet_optim_get_state", key);
  if (wi < 0) return wi;
  if (!n->d_m) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_optim_get_state: no optimizer state yet");
  const size_t bytes = numel(n->wts[wi].shape) * sizeof(float);
  HIPCHK(nullptr, hipDeviceSynchronize());
  if (exp_avg_host) HIPCHK(nullptr, hipMemcpy(exp_avg_host, n->d_m + n->poff[wi], bytes, hipMemcpyDeviceToHost));
  if (exp_avg_sq_host) HIPCHK(nullptr, hipMemcpy(exp_avg_sq_host, n->d_v + n->poff[wi], bytes, hipMemcpyDeviceToHost));
  if (step) *step = n->opt_step;
  return FDSR_OK;
}

int fdsr_nafnet_optim_set_state(fdsr_nafnet n, const char* key, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t step) {
  const int wi = find_weight(n, "fdsr_nafnet_optim_set_state", key);
  if (wi < 0) return wi;
  if (step < 0) return fail(nullptr, FDSR_E_INVALID, "fdsr_nafnet_optim_set_state: negative step");
  for (const WT& w : n->wts)
    if (!w.loaded) return fail(nullptr, FDSR_E_STATE, "fdsr_nafnet_optim_set_state: tensor '%s' is missing", w.key.c_str());
  int rc = finalize(n);
  if (rc) return rc;
  if ((rc = ensure_train(n))) return rc;
  const size_t bytes = numel(n->wts[wi].shape) * sizeof(float);
  HIPCHK(nullptr, hipDeviceSynchronize());
  if (exp_avg_host) HIPCHK(nullptr, hipMemcpy(n->d_m + n->poff[wi], exp_avg_host, bytes, hipMemcpyHostToDevice));
  if (exp_avg_sq_host) HIPCHK(nullptr, hipMemcpy(n->d_v + n->poff[wi], exp_avg_sq_host, bytes, hipMemcpyHostToDevice));
  n->opt_step = step;
  return FDSR_OK;
}

}  // extern "C"
