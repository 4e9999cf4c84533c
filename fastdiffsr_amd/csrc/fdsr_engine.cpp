// Host side of libfdsr_hip.so: checkpoint repacking, workspace planning, running
// the plan of the UNet and the C ABI (include/fdsr.h).  The static plan itself (ops,
// tensors, weight schema) is built in fdsr_plan.cpp, the sampling loop in fdsr_sample.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "fdsr_engine_int.h"
#include "fdsr_train.h"

using namespace fdsr;
using namespace fdsr_int;

namespace fdsr_int {
thread_local std::string g_global_error;

int fail(fdsr_handle h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_global_error = buf;
  return code;
}
}  // namespace fdsr_int

namespace fdsr_int {

int ensure_device(fdsr_handle h) {
  if (h->d_params) return FDSR_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(h, FDSR_E_HIP, "no HIP device visible: the FastDiffSR engine has no CPU fallback");
  HIPCHK(h, hipMalloc((void**)&h->d_params, h->param_floats * sizeof(float)));
  HIPCHK(h, hipMemset(h->d_params, 0, h->param_floats * sizeof(float)));
  if (!h->sr3) {
  // unet.py:27-31: step = arange(count)/count ; exp(-ln(1e4) * step), in fp32
    const int half = h->freq_count;
    std::vector<float> fr(half);
    for (int k = 0; k < half; ++k) {
      const float step = (float)k / (float)half;
      fr[k] = expf((float)(-std::log(1e4)) * step);
      // gdp_modules/unet.py:130-132: exp(-log(max_period) * arange(half) / half): multiply first, then divide (fp32)
      if (h->gdp) fr[k] = expf(((float)(-std::log(1e4)) * (float)k) / (float)half);
    }
    HIPCHK(h, hipMemcpy(h->d_params + h->weights[h->w_freq].dev_off, fr.data(), half * sizeof(float), hipMemcpyHostToDevice));
  }
  HIPCHK(h, hipMalloc((void**)&h->d_master, std::max<size_t>(h->master_floats, 4) * sizeof(float)));
  HIPCHK(h, hipMemset(h->d_master, 0, std::max<size_t>(h->master_floats, 4) * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->d_hscale, h->weights.size() * 2 * sizeof(float)));
  {
    std::vector<float> ones(h->weights.size() * 2, 1.0f);
    HIPCHK(h, hipMemcpy(h->d_hscale, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  HIPCHK(h, hipMalloc((void**)&h->d_sat, 64));
  HIPCHK(h, hipMemset(h->d_sat, 0, 64));
  if (h->wq_bytes) {
    HIPCHK(h, hipMalloc((void**)&h->d_wq, h->wq_bytes));
    HIPCHK(h, hipMemset(h->d_wq, 0, h->wq_bytes));
  }
  if (!h->kernels_ready) {
    HIPCHK(h, kernels_init());
    HIPCHK(h, kernels_h_init());
    HIPCHK(h, kernels_tail_init());
    h->kernels_ready = true;
  }
  return FDSR_OK;
}

struct Block { size_t off, size; bool free; };

// Workspace plan for (N,H,W): stats | temb | gate | activation arena (liveness-reused).
int make_shape_plan(fdsr_handle h, int N, int H, int W, ShapePlan* sp) {
  const int down = 1 << (h->cfg.n_mults - 1);
  if (N < 1 || H < down || W < down || H % down || W % down)
    return fail(h, FDSR_E_INVALID, "batch>=1 and H,W multiples of %d required (got %d,%d,%d)", down, N, H, W);
  sp->N = N; sp->H = H; sp->W = W; sp->debug = h->debug;
  sp->tun_epoch = g_tun.epoch;
  size_t off = 0;
  sp->gn_off.assign(h->n_gn_slots, 0);
  for (const Op& op : h->ops)
    if (op.kind == Op::GN_FINALIZE) {
      sp->gn_off[op.gn_slot] = off;
      off += align_up((size_t)2 * N * (op.C0 + op.C1) * sizeof(float), 256);
    }
  sp->training = h->training;
  sp->drop_off.assign(h->n_drop_slots, 0);
  if (h->training)
    for (const Op& op : h->ops)
      if (op.kind == Op::CONV && op.drop_slot >= 0) {
        sp->drop_off[op.drop_slot] = off;
        off += align_up((size_t)N * (H >> op.lvl_in) * (W >> op.lvl_in) * op.C0, 256);
      }
  if (h->training && h->n_drop_slots > 0) {
    size_t mx = 0;
    for (const Op& op : h->ops)
      if (op.kind == Op::CONV && op.drop_slot >= 0) mx = std::max(mx, (size_t)N * (H >> op.lvl_in) * (W >> op.lvl_in) * op.C0 * sizeof(float));
    sp->off_dropA = off;
    off += align_up(mx, 256);
  }
  sp->gn_stats_off.assign(h->n_gn_slots, 0);
  for (int g = 0; g < h->n_gn_slots; ++g) {
    sp->gn_stats_off[g] = off;
    off += align_up((size_t)N * h->cfg.norm_groups * 2 * sizeof(float), 256);
  }
  sp->off_temb = off;  off += align_up((size_t)N * h->TE * sizeof(float), 256);
  {
    size_t gate_floats = 1;
    for (const Op& op : h->ops)
      if (op.kind == Op::CLAM)
        gate_floats = std::max(gate_floats, clam_slam_scratch_floats(N, (H >> op.lvl_in) * (W >> op.lvl_in), op.C0));
    sp->off_gate = off;  off += align_up(gate_floats * sizeof(float), 256);
  }
  // small grids split the K loop over workgroups; the slices meet in a scratch region
  sp->op_ksplit.assign(h->ops.size(), 1);
  size_t sk_bytes = 0;
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const Op& op = h->ops[i];
    if (op.kind != Op::CONV || !h->weights[op.w].h_ok) continue;
    const WeightEntry& w = h->weights[op.w];
    const int Ho = H >> op.lvl_out, Wo = W >> op.lvl_out;
    const int sk = conv_h_ksplit(op.ck, N, Ho, Wo, op.Cout, w.h_cout_pad, w.h_cin_pad, op.C0, op.C1);
    sp->op_ksplit[i] = sk;
    if (sk > 1) sk_bytes = std::max(sk_bytes, (size_t)sk * N * Ho * Wo * op.Cout * sizeof(float));
  }
  sp->off_splitk = off;  off += align_up(sk_bytes, 256);
  sp->gsum_off.assign(h->tensors.size(), 0);
  sp->tensor_gsum.assign(h->tensors.size(), 0);
  sp->off_gsum = off;
  for (size_t t = 0; t < h->tensors.size(); ++t)
    if (h->tensors[t].need_part && h->tensors[t].C > 0 && !(h->tensors[t].C & 1)) {
      sp->gsum_off[t] = off;
      off += align_up((size_t)N * (h->tensors[t].C / 2) * GSUM_SHARDS * 2 * sizeof(unsigned long long), 256);
    }
  sp->gsum_bytes = off - sp->off_gsum;
  // which tensors are read by a GroupNorm'd conv that lands on a consumer-side kernel at this shape (a pure function of the shapes, as
  // the split factor above): only their producers add pair sums (a large batch's producers would add them for nobody)
  for (int prec = PREC_F16X3; prec <= PREC_F16; ++prec) {
    sp->gsum_wanted[prec].assign(h->tensors.size(), 0);
    for (size_t i = 0; i < h->ops.size(); ++i) {
      const Op& op = h->ops[i];
      if (op.kind != Op::CONV || op.gn_slot < 0 || op.ck != CONV3_S1 || !h->weights[op.w].h_ok || op.gn_plain) continue;
      const WeightEntry& w = h->weights[op.w];
      ConvParams q{};
      q.N = N; q.Hin = q.Hout = H >> op.lvl_out; q.Win = q.Wout = W >> op.lvl_out;
      q.C0 = op.C0; q.C1 = op.C1; q.Cout = op.Cout; q.Cin_pad = w.h_cin_pad; q.Cout_pad = w.h_cout_pad;
      q.ksplit = sp->op_ksplit[i];
      q.gs_G = h->cfg.norm_groups;
      q.gs_gamma = q.gs_beta = reinterpret_cast<const float*>(sp);      // (non-null stand-ins: only the shape fields are read)
      q.gs0 = reinterpret_cast<const unsigned long long*>(sp);
      q.res = op.res >= 0 ? reinterpret_cast<const float*>(sp) : nullptr;
      if (op.rider >= 0) {                                               // (a rider changes which forms take the launch)
        const Op& kr = h->ops[op.rider];
        q.xr0 = reinterpret_cast<const float*>(sp); q.Cr0 = kr.C0; q.Cr1 = kr.C1; q.nkr = h->weights[kr.w].h_cin_pad / 16;
        q.res = nullptr;
      }
      if (!conv_h_gnc_ok(op.ck, prec, q)) continue;
      sp->gsum_wanted[prec][op.src0] = 1;
      if (op.src1 >= 0) sp->gsum_wanted[prec][op.src1] = 1;
    }
  }
  const size_t arena0 = off;
  sp->tensor_off.assign(h->tensors.size(), 0);
  sp->part_off.assign(h->tensors.size(), 0);
  sp->tensor_nt.assign(h->tensors.size(), 0);
  auto act_bytes = [&](const TensorDesc& t) {
    const size_t hw = (size_t)(H >> t.level) * (W >> t.level);
    if (t.C < 0) return align_up(attn_scratch_floats(N, (int)hw, -t.C) * sizeof(float), 256);   // attention scores of |C| heads
    return align_up((size_t)N * hw * t.C * sizeof(float), 256);
  };
  auto part_bytes = [&](const TensorDesc& t) -> size_t {
    if (!t.need_part) return 0;
    const int mt = conv_max_tiles(H >> t.level, W >> t.level);
    return align_up((size_t)N * mt * t.C * 2 * sizeof(float), 256);
  };
  auto tbytes = [&](const TensorDesc& t) { return act_bytes(t) + part_bytes(t); };
  std::vector<Block> blocks;
  size_t arena_end = 0;
  auto alloc = [&](size_t need) -> size_t {
    for (size_t i = 0; i < blocks.size(); ++i)
      if (blocks[i].free && blocks[i].size >= need) {
        if (blocks[i].size > need) {
          Block rest{blocks[i].off + need, blocks[i].size - need, true};
          blocks[i].size = need;
          blocks.insert(blocks.begin() + i + 1, rest);
        }
        blocks[i].free = false;
        return blocks[i].off;
      }
    if (!blocks.empty() && blocks.back().free) {   // grow the trailing free block
      blocks.back().size = need;
      blocks.back().free = false;
      arena_end = blocks.back().off + need;
      return blocks.back().off;
    }
    blocks.push_back(Block{arena_end, need, false});
    arena_end += need;
    return blocks.back().off;
  };
  auto release = [&](size_t o) {
    for (size_t i = 0; i < blocks.size(); ++i)
      if (blocks[i].off == o && !blocks[i].free) {
        blocks[i].free = true;
        if (i + 1 < blocks.size() && blocks[i + 1].free) { blocks[i].size += blocks[i + 1].size; blocks.erase(blocks.begin() + i + 1); }
        if (i > 0 && blocks[i - 1].free) { blocks[i - 1].size += blocks[i].size; blocks.erase(blocks.begin() + i); }
        return;
      }
  };
  // persistent tensors first
  for (size_t t = 0; t < h->tensors.size(); ++t)
    if (h->tensors[t].persistent) sp->tensor_off[t] = alloc(tbytes(h->tensors[t]));
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const Op& op = h->ops[i];
    if (op.aux >= 0 && h->tensors[op.aux].first_def == (int)i) sp->tensor_off[op.aux] = alloc(tbytes(h->tensors[op.aux]));
    if (op.dst >= 0 && !h->tensors[op.dst].persistent && h->tensors[op.dst].first_def == (int)i)
      sp->tensor_off[op.dst] = alloc(tbytes(h->tensors[op.dst]));
    if (!h->debug)
      for (size_t t = 0; t < h->tensors.size(); ++t)
        if (!h->tensors[t].persistent && h->tensors[t].last_use == (int)i && h->tensors[t].first_def >= 0)
          release(sp->tensor_off[t]);
  }
  for (auto& o : sp->tensor_off) o += arena0;
  for (size_t t = 0; t < h->tensors.size(); ++t)
    if (h->tensors[t].need_part) sp->part_off[t] = sp->tensor_off[t] + act_bytes(h->tensors[t]);
  sp->bytes = arena0 + arena_end;
  return FDSR_OK;
}

int get_plan(fdsr_handle h, int N, int H, int W) {
  if (h->plan.N == N && h->plan.H == H && h->plan.W == W && h->plan.debug == h->debug && h->plan.training == h->training &&
      h->plan.tun_epoch == g_tun.epoch && h->plan.bytes)
    return FDSR_OK;
  ShapePlan sp;
  int rc = make_shape_plan(h, N, H, W, &sp);
  if (rc) return rc;
  h->plan = sp;
  return FDSR_OK;
}

double conv_flops(const Op& op, int N, int H, int W) {
  const int ks = op.ck == CONV1 ? 1 : 3;
  const double px = (double)N * (H >> op.lvl_out) * (W >> op.lvl_out);
  // algorithmic: real input channels (the packed input counts its 6 real channels)
  return 2.0 * px * op.Cout * (double)(op.C0 + op.C1) * ks * ks;
}

// One UNet forward over the plan; input already packed in tensor t_in.
int run_unet(fdsr_handle h, int N, int H, int W, char* ws, const float* nl_dev, float nl_scalar, hipStream_t st,
             const float* temb_row) {
  ShapePlan& sp = h->plan;
  const int G = h->cfg.norm_groups;
  const float* temb = temb_row ? temb_row : reinterpret_cast<const float*>(ws + sp.off_temb);
  float* gate = reinterpret_cast<float*>(ws + sp.off_gate);
  auto P = [&](int widx) -> const float* { return widx >= 0 ? h->d_params + h->weights[widx].dev_off : nullptr; };
  auto TP = [&](int t) -> float* { return t >= 0 ? reinterpret_cast<float*>(ws + sp.tensor_off[t]) : nullptr; };

  auto PART = [&](int t) -> float* { return (t >= 0 && sp.part_off[t]) ? reinterpret_cast<float*>(ws + sp.part_off[t]) : nullptr; };
  if (!temb_row) {
    int rc = fill_temb(h, reinterpret_cast<float*>(ws + sp.off_temb), N, nl_dev, nl_scalar, st);
    if (rc) return rc;
  }
  // consumer-side GroupNorm: sampling forwards of the 16-bit modes only (a training forward keeps the statistics for its backward; a debug
  // forward -- every layer in a buffer of its own -- takes the same kernels as a plain one, so the two stay bitwise equal); the
  // producers' tables start from zero
  bool gsum_any = false;
  if (h->prec != PREC_F32)
    for (char c : sp.gsum_wanted[h->prec]) gsum_any |= c != 0;
  const bool gsum_on = g_tun.gn_consumer && h->prec != PREC_F32 && !h->training && !h->keep_stats && sp.gsum_bytes > 0 &&
                       gsum_any && !(g_tun.knockout & 1);
  auto GSUM = [&](int t) -> unsigned long long* {
    return (gsum_on && t >= 0 && sp.gsum_off[t] && sp.gsum_wanted[h->prec][t]) ? reinterpret_cast<unsigned long long*>(ws + sp.gsum_off[t]) : nullptr;
  };
  std::fill(sp.tensor_gsum.begin(), sp.tensor_gsum.end(), 0);
  if (gsum_on) HIPCHK(h, hipMemsetAsync(ws + sp.off_gsum, 0, sp.gsum_bytes, st));
  int pending_gn = -1;              // a GN_FINALIZE op whose launch waits for its consumer's verdict (index into h->ops)
  auto launch_finalize = [&](const Op& op) -> int {
    const int Hi = H >> op.lvl_in, Wi = W >> op.lvl_in;
    GnFinalizeParams g{};
    g.part0 = PART(op.src0); g.nt0 = sp.tensor_nt[op.src0]; g.C0 = op.C0;
    g.part1 = PART(op.src1); g.nt1 = op.src1 >= 0 ? sp.tensor_nt[op.src1] : 0; g.C1 = op.C1;
    if (!g.part0 || g.nt0 <= 0 || (op.src1 >= 0 && (!g.part1 || g.nt1 <= 0)))
      return fail(h, FDSR_E_STATE, "internal: GroupNorm input of %s has no partial sums", op.name.c_str());
    g.gamma = P(op.gamma); g.beta = P(op.beta);
    g.scale = reinterpret_cast<float*>(ws + sp.gn_off[op.gn_slot]);
    g.shift = g.scale + (size_t)N * (op.C0 + op.C1);
    g.stats = h->keep_stats ? reinterpret_cast<float*>(ws + sp.gn_stats_off[op.gn_slot]) : nullptr;
    if (op.film_off >= 0) { g.film = temb; g.film_stride = temb_row ? 0 : h->TE; g.film_off = op.film_off; }
    g.N = N; g.G = G; g.HW = Hi * Wi; g.eps = 1e-5f;
    if (!(g_tun.knockout & 1)) HIPCHK(h, launch_gn_finalize(g, st));   // (knockout: timing-only probe, results are garbage)
    return FDSR_OK;
  };
  const bool dropout_on = h->training && h->n_drop_slots > 0;
  if (dropout_on) {
    if (prec_is16(h->prec))
      return fail(h, FDSR_E_INVALID, "train mode with dropout runs on the fp32-grade kernels: fdsr_set_precision(FDSR_PREC_F32 or _F16X3)");
    h->drop_step += 1;
  }
  for (size_t oi = 0; oi < h->ops.size(); ++oi) {
    const Op& op = h->ops[oi];
    const int Hi = H >> op.lvl_in, Wi = W >> op.lvl_in;
    if (pending_gn >= 0 && op.kind != Op::CONV && op.kind != Op::GN_FINALIZE) {   // (only a conv can stand in for the finalisation)
      int rc = launch_finalize(h->ops[pending_gn]); if (rc) return rc; pending_gn = -1;
    }
    switch (op.kind) {
      case Op::GN_FINALIZE: {
        if (pending_gn >= 0) { int rc = launch_finalize(h->ops[pending_gn]); if (rc) return rc; pending_gn = -1; }
        // Where every source's producer filled its table of pair sums, the launch waits for the consumer conv (the next op of this
        // GroupNorm slot): a consumer that forms scale / shift itself (conv_h_gnc_ok) makes it unnecessary
        const bool tabled = gsum_on && op.film_off < 0 && sp.tensor_gsum[op.src0] && (op.src1 < 0 || sp.tensor_gsum[op.src1]);
        if (tabled) pending_gn = (int)oi;
        else { int rc = launch_finalize(op); if (rc) return rc; }
        break;
      }
      case Op::CONV: {
        // ResnetBlock's res_conv as a rider of block2 (16-bit kernels, sampling): one launch, no round trip of its output
        // through HBM.  Measured same-box: every res_conv fused is as good as or better than fusing only the bandwidth-bound
        // ones (FDSR_RIDER=1: full-resolution level + input widths up to the output width), at every batch size;
        // FDSR_RIDER=0 turns it off.  Training forwards ride too (the backward never reads the res_conv output).
        auto rides = [&](const Op& k2) -> bool {
          const int mode = g_tun.rider;
          if (mode == 0 || k2.rider < 0 || h->prec == PREC_F32) return false;
          const Op& kr = h->ops[k2.rider];
          const WeightEntry &w2 = h->weights[k2.w], &wr = h->weights[kr.w];
          if (!w2.h_ok || !wr.h_ok || wr.h_WN != w2.h_WN || wr.h_cout_pad != w2.h_cout_pad) return false;
          if (mode == 3) return k2.lvl_out != 0;   // everywhere but the full-resolution level (whose 16-row rider tile is the slowest kernel of the loop)
          return mode == 2 || k2.lvl_out == 0 || kr.C0 + kr.C1 <= k2.Cout;
        };
        if (op.rider_of >= 0 && rides(h->ops[op.rider_of])) break;
        const bool ridden = op.rider >= 0 && rides(op);
        ConvParams p{};
        const WeightEntry& w = h->weights[op.w];
        p.x0 = TP(op.src0);
        p.x1 = TP(op.src1);
        p.w = P(op.w);
        p.bias = op.b == -2 ? P(h->w_zero_bias) : P(op.b);
        p.temb = op.temb_off >= 0 ? temb : nullptr;
        p.temb_stride = temb_row ? 0 : h->TE;
        p.temb_off = op.temb_off >= 0 ? op.temb_off : 0;
        p.res = TP(op.res);
        p.out = TP(op.dst);
        if (ridden) {
          const Op& kr = h->ops[op.rider];
          const WeightEntry& wr = h->weights[kr.w];
          p.res = nullptr;
          p.xr0 = TP(kr.src0); p.xr1 = TP(kr.src1); p.Cr0 = kr.C0; p.Cr1 = kr.C1;
          p.nkr = wr.h_cin_pad / 16;
          p.wq_r = h->d_wq + wr.hq_off[prec_wform(h->prec)];
          p.bias_r = P(kr.b);
          p.w_inv_scale_r = wr.h_inv_scale[prec_wform(h->prec)];
          if (prec_wform(h->prec) == PREC_F16X3) p.w_inv_scale_r_dev = h->d_hscale + 2 * (size_t)kr.w + 1;
        }
        if (op.gn_slot >= 0) {
          p.gn_scale = reinterpret_cast<const float*>(ws + sp.gn_off[op.gn_slot]);
          p.gn_shift = p.gn_scale + (size_t)N * (op.C0 + op.C1);
          p.gn_plain = op.gn_plain ? 1 : 0;   // attn.qkv: SelfAttention.norm has no Swish
        }
        p.part_out = op.no_part ? nullptr : PART(op.dst);   // res_conv output is overwritten in place by block2
        if (dropout_on && op.drop_slot >= 0) {              // Dropout(p) between Swish and this conv (train mode)
          unsigned char* mask = reinterpret_cast<unsigned char*>(ws + sp.drop_off[op.drop_slot]);
          HIPCHK(h, launch_dropout_mask(mask, (size_t)N * Hi * Wi * op.C0, h->drop_seed, h->drop_step, (unsigned)op.drop_slot,
                                        h->cfg.dropout, st, (size_t)g_tun.drop_image_offset * Hi * Wi * op.C0));
          // the fp32 kernel and the f16x3 16x16x32 kernels apply the mask in their staging; a 16-bit launch that lands elsewhere reads
          // the materialised dropped activation raw (decided below, once the launch's shape fields are set)
          p.drop_mask = mask;
          p.drop_scale = 1.0f / (1.0f - h->cfg.dropout);
        }
        // bf16 mode keeps every activation but the packed input and eps as bf16 in HBM
        p.out_f32 = (op.dst == h->t_eps) ? 1 : 0;
        p.out_bf16 = op.dst != h->t_eps ? prec_act16(h->prec) : 0;
        int nt = 0;
        p.N = N; p.Hin = Hi; p.Win = Wi;
        p.Hout = H >> op.lvl_out; p.Wout = W >> op.lvl_out;
        p.C0 = op.C0; p.C1 = op.C1; p.Cout = op.Cout;
        p.Cin_pad = w.cin_pad; p.Cout_pad = w.cout_pad;
        if (p.drop_mask && h->prec != PREC_F32) {
          ConvParams t = p;                    // as launch_conv_h will see it
          t.Cin_pad = w.h_cin_pad; t.Cout_pad = w.h_cout_pad;
          t.ksplit = sp.op_ksplit[oi];
          const bool staged = g_tun.drop_stage && h->prec == PREC_F16X3 && w.h_ok && op.ck == CONV3_S1 && conv_h_drop_ok(op.ck, h->prec, t);
          if (!staged) {
            float* a = reinterpret_cast<float*>(ws + sp.off_dropA);
            HIPCHK(h, launch_gn_silu_drop(p.x0, p.gn_scale, p.gn_shift, p.drop_mask, p.drop_scale, a, N, Hi * Wi, op.C0, st));
            p.x0 = a;
            p.gn_scale = p.gn_shift = nullptr;
            p.drop_mask = nullptr;
          }
        }
        const bool timed = h->profiling && h->prof_step && op.ck != CONV1;
        if (timed) {
          if (h->ev_used + 2 > h->ev_pool.size()) {
            for (int k = 0; k < 256; ++k) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); h->ev_pool.push_back(e); }
          }
          HIPCHK(h, hipEventRecord(h->ev_pool[h->ev_used++], st));
        }
        // consumer-side GroupNorm: the finalisation of this conv's GroupNorm is still pending (its sources carry tables of pair sums):
        // a launch that lands on a GNC kernel forms scale / shift itself; anything else gets the finalisation launch now
        bool gnc = false;
        ConvParams gcp{};
        if (pending_gn >= 0) {
          const Op& gop = h->ops[pending_gn];
          if (op.gn_slot >= 0 && gop.gn_slot == op.gn_slot && h->prec != PREC_F32 && w.h_ok && op.ck == CONV3_S1 && !p.drop_mask) {
            gcp = p;
            gcp.Cin_pad = w.h_cin_pad; gcp.Cout_pad = w.h_cout_pad;
            gcp.ksplit = sp.op_ksplit[oi];
            gcp.gn_scale = gcp.gn_shift = nullptr;
            gcp.gs0 = GSUM(gop.src0); gcp.gs1 = GSUM(gop.src1);
            gcp.gs_gamma = P(gop.gamma); gcp.gs_beta = P(gop.beta); gcp.gs_eps = 1e-5f; gcp.gs_G = G;
            gnc = gcp.gs0 && (gop.src1 < 0 || gcp.gs1) && conv_h_gnc_ok(op.ck, h->prec, gcp);
          }
          if (!gnc) { int rc = launch_finalize(gop); if (rc) return rc; }
          pending_gn = -1;
        }
        // the two ends of the UNet in the 16-bit modes: bandwidth-shaped kernels of their own (fdsr_conv_tail.hip), weights read
        // from the fp32 master copy (always current, also right after optimiser steps)
        const float* wmaster = h->master_off[op.w] != SIZE_MAX ? h->d_master + h->master_off[op.w] : nullptr;
        const int* satf = (h->prec == PREC_F16X3 && g_tun.sat_guard) ? h->d_sat : nullptr;
        if (h->prec != PREC_F32 && wmaster && op.src0 == h->t_in && h->CP == 8 &&
            conv_in8_ok(op.ck, h->prec, p, (int)w.shape[1])) {
          p.sat_flag = const_cast<int*>(satf);
          HIPCHK(h, launch_conv_in8(h->prec, p, wmaster, (int)w.shape[1], st, &nt));
        } else if (h->prec != PREC_F32 && wmaster && w.h_ok && conv_out3_ok(op.ck, h->prec, p)) {
          HIPCHK(h, launch_conv_out3(h->prec, p, wmaster, (int)w.shape[1], st, &nt));
        } else if (h->prec != PREC_F32 && w.h_ok) {
          p.sat_flag = (h->prec == PREC_F16X3 && g_tun.sat_guard) ? h->d_sat : nullptr;
          p.wq = h->d_wq + w.hq_off[prec_wform(h->prec)];
          p.w_inv_scale = w.h_inv_scale[prec_wform(h->prec)];
          p.Cin_pad = w.h_cin_pad;
          p.Cout_pad = w.h_cout_pad;
          if (prec_wform(h->prec) == PREC_F16X3) p.w_inv_scale_dev = h->d_hscale + 2 * (size_t)op.w + 1;
          // (a sub-pixel form that lags, or has two scale sources after a single-tensor load: the generic kernel)
          const fdsr_forms::Up2 up2 = fdsr_forms::up2_form(h->forms, h->prec);
          if (op.ck == CONV3_UP && g_tun.up2 && !op.force_generic && up2 != fdsr_forms::UP2_GENERIC) {
            p.w_inv_scale_dev = up2 == fdsr_forms::UP2_DEVICE_SCALE ? h->d_up2_inv + op.w : nullptr;
            p.wq = h->d_wq + w.up2_off[prec_wform(h->prec)];
            p.w_inv_scale = w.up2_inv_scale[prec_wform(h->prec)];
            if (gsum_on && p.part_out && GSUM(op.dst) && conv_h_gsum_ok(CONV3_UP, h->prec, p, true)) {
              p.gsum_out = GSUM(op.dst);
              sp.tensor_gsum[op.dst] = 1;
            }
            HIPCHK(h, launch_conv_up2_h(h->prec, p, st, &nt));
          } else {
            p.ksplit = (op.ck == CONV3_UP) ? 1 : sp.op_ksplit[oi];
            p.kscratch = reinterpret_cast<float*>(ws + sp.off_splitk);
            if (gnc) {   // scale / shift from the sources' tables, in the kernel's prologue
              p.gn_scale = p.gn_shift = nullptr;
              p.gs0 = gcp.gs0; p.gs1 = gcp.gs1; p.gs_gamma = gcp.gs_gamma; p.gs_beta = gcp.gs_beta; p.gs_eps = gcp.gs_eps; p.gs_G = gcp.gs_G;
            }
            if (gsum_on && p.part_out && GSUM(op.dst) && conv_h_gsum_ok(op.ck, h->prec, p, false)) {
              p.gsum_out = GSUM(op.dst);
              sp.tensor_gsum[op.dst] = 1;
            }
            HIPCHK(h, launch_conv_h(op.ck, h->prec, p, st, &nt));
          }
        } else {
          HIPCHK(h, launch_conv(op.ck, p, st, &nt));
        }
        sp.tensor_nt[op.dst] = nt;
        if (timed) {
          HIPCHK(h, hipEventRecord(h->ev_pool[h->ev_used++], st));
          double f = conv_flops(op, N, H, W);
          if (ridden) f += conv_flops(h->ops[op.rider], N, H, W);
          if (op.src0 == h->t_in) f *= (double)h->cfg.in_channel / h->CP;
          h->prof_flops += f;
          // algorithmic bytes (ideal-fused): every input element read once, the output written once, the residual read
          // once, in the element size the active mode keeps that tensor in (bf16 mode: 2 bytes for everything but the packed
          // network input and eps), plus the GroupNorm partial-sum appendix this launch writes (it stands where 8d has a second
          // read of each GroupNorm input: [N][tiles][Cout][2] fp32)
          const double esz = prec_is16(h->prec) ? 2.0 : 4.0;
          const double esz_in = op.src0 == h->t_in ? 4.0 : esz, esz_out = p.out_f32 ? 4.0 : esz;
          const double out_elems = (double)N * p.Hout * p.Wout * op.Cout;
          h->prof_bytes += esz_in * N * (double)Hi * Wi * (op.src0 == h->t_in ? h->CP : op.C0 + op.C1) + esz_out * out_elems;
          if (ridden) h->prof_bytes += esz * N * (double)Hi * Wi * (h->ops[op.rider].C0 + h->ops[op.rider].C1);
          else if (op.res >= 0) h->prof_bytes += esz * out_elems;
          if (p.part_out) h->prof_bytes += 8.0 * N * (double)nt * op.Cout;
        }
        break;
      }
      case Op::ATTN: {
        HIPCHK(h, launch_self_attention(TP(op.src0), TP(op.aux), TP(op.dst), N, Hi * Wi, op.C0, op.heads, st, prec_act16(h->prec)));
        break;
      }
      case Op::POOL2: {
        const float* sc = op.gn_slot >= 0 ? reinterpret_cast<const float*>(ws + sp.gn_off[op.gn_slot]) : nullptr;
        HIPCHK(h, launch_pool2(TP(op.src0), sc, sc ? sc + (size_t)N * op.C0 : nullptr, TP(op.dst), N, Hi, Wi, op.C0, st, prec_act16(h->prec)));
        break;
      }
      case Op::UP2X:
        HIPCHK(h, launch_upsample2(TP(op.src0), TP(op.dst), N, Hi, Wi, op.C0, st, prec_act16(h->prec)));
        break;
      case Op::CLAM:
        HIPCHK(h, launch_clam_gate(TP(op.src0), N, Hi * Wi, op.C0, P(op.fc1), P(op.fc2), op.C0 / 16, gate, st,
                                   prec_act16(h->prec)));
        break;
      case Op::SLAM: {
        int nt = 0;
        HIPCHK(h, launch_slam(TP(op.src0), gate, P(op.w), N, Hi, Wi, op.C0, TP(op.dst), PART(op.dst), st, &nt,
                              prec_act16(h->prec)));
        sp.tensor_nt[op.dst] = nt;
        break;
      }
    }
  }
  if (pending_gn >= 0) { int rc = launch_finalize(h->ops[pending_gn]); if (rc) return rc; }
  return FDSR_OK;
}

int check_ready(fdsr_handle h, bool need_schedule) {
  for (const auto& w : h->weights)
    if (w.live && !w.loaded) return fail(h, FDSR_E_STATE, "weight '%s' has not been loaded", w.key.c_str());
  if (need_schedule && h->T <= 0) return fail(h, FDSR_E_STATE, "fdsr_set_schedule has not been called");
  return FDSR_OK;
}

// the weights are loaded (and a schedule set), the plan is the one of (N,H,W), and the workspace holds it
int plan_ready(fdsr_handle h, bool need_schedule, int N, int H, int W, void* ws, size_t bytes) {
  int rc = check_ready(h, need_schedule);
  if (rc) return rc;
  if ((rc = get_plan(h, N, H, W))) return rc;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return fail(h, FDSR_E_WORKSPACE, "workspace must be a 256-byte aligned device pointer");
  if (bytes < h->plan.bytes) return fail(h, FDSR_E_WORKSPACE, "workspace too small: %zu < %zu bytes", bytes, h->plan.bytes);
  return FDSR_OK;
}

}  // namespace fdsr_int

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

#ifndef FDSR_SRC_SHA256
#define FDSR_SRC_SHA256 "unstamped"
#endif
// ends with the SHA-256 of the sources this binary was built from (fastdiffsr_amd/build.py: source_hash)
const char* fdsr_version(void) {
  return "fdsr-hip 0.4 (gfx950; NHWC implicit-GEMM MFMA convolutions: f16x3 / f32 / bf16) FDSR_SRC_SHA256=" FDSR_SRC_SHA256;
}

const char* fdsr_last_error(fdsr_handle h) { return h ? h->err.c_str() : g_global_error.c_str(); }

int fdsr_create(const fdsr_config* cfg, fdsr_handle* out) {
  if (!cfg || !out) return fail(nullptr, FDSR_E_INVALID, "null argument");
  fdsr_engine* h = new fdsr_engine();
  h->cfg = *cfg;
  int rc = build_plan(h);
  if (rc) {
    g_global_error = h->err;
    delete h;
    return rc;
  }
  *out = h;
  return FDSR_OK;
}

void fdsr_destroy(fdsr_handle h) {
  if (!h) return;
  drop_captures(h);
  for (auto e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->d_params) (void)hipFree(h->d_params);
  if (h->d_wq) (void)hipFree(h->d_wq);
  if (h->d_sat) (void)hipFree(h->d_sat);
  if (h->h_sat) (void)hipHostFree(h->h_sat);
  if (h->d_temb_table) (void)hipFree(h->d_temb_table);
  if (h->d_nl) (void)hipFree(h->d_nl);
  if (h->d_rng) (void)hipFree(h->d_rng);
  for (void* q : {(void*)h->d_step_ctl, (void*)h->d_step_row, (void*)h->d_step_sched})
    if (q) (void)hipFree(q);
  if (h->d_wtq) (void)hipFree(h->d_wtq);
  if (h->d_hamax) (void)hipFree(h->d_hamax);
  if (h->d_copy_tab) (void)hipFree(h->d_copy_tab);
  if (h->d_up2_inv) (void)hipFree(h->d_up2_inv);
  for (float* q : {h->d_master, h->d_grad, h->d_adam_m, h->d_adam_v, h->d_wt, h->d_zero, h->d_hscale})
    if (q) (void)hipFree(q);
  delete h;
}

int fdsr_num_weights(fdsr_handle h) {
  if (!h) return FDSR_E_INVALID;
  return h->n_schema;   // without the synthetic entries (frequency table, zero bias)
}

int fdsr_weight_info(fdsr_handle h, int idx, char* key, int key_cap, int64_t shape[4], int* ndim, int* live) {
  if (!h || idx < 0 || idx >= fdsr_num_weights(h)) return fail(h, FDSR_E_INVALID, "weight index out of range");
  const WeightEntry& w = h->weights[idx];
  if (key && key_cap > 0) {
    strncpy(key, w.key.c_str(), key_cap - 1);
    key[key_cap - 1] = 0;
  }
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = i < (int)w.shape.size() ? w.shape[i] : 1;
  if (ndim) *ndim = (int)w.shape.size();
  if (live) *live = w.live ? 1 : 0;
  return FDSR_OK;
}

int fdsr_load_weight(fdsr_handle h, const char* key, const float* host, const int64_t* shape, int ndim) {
  if (!h || !key || !host || !shape) return fail(h, FDSR_E_INVALID, "null argument");
  auto it = h->key2w.find(key);
  if (it == h->key2w.end()) return fail(h, FDSR_E_KEY, "unexpected key '%s'", key);
  WeightEntry& w = h->weights[it->second];
  if (ndim != (int)w.shape.size()) return fail(h, FDSR_E_KEY, "'%s': rank %d, expected %zu", key, ndim, w.shape.size());
  for (int i = 0; i < ndim; ++i)
    if (shape[i] != w.shape[i]) return fail(h, FDSR_E_KEY, "'%s': dim %d is %lld, expected %lld", key, i, (long long)shape[i], (long long)w.shape[i]);
  if (!w.live) { w.loaded = true; return FDSR_OK; }   // never executed (unet.py:212): schema only
  int rc = ensure_device(h);
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(h->d_master + h->master_off[it->second], host, numel(w.shape) * sizeof(float), hipMemcpyHostToDevice));
  if ((rc = pack_weight_host(h, w, host))) return rc;
  w.loaded = true;
  return apply_plan(h, fdsr_forms::on_load(h->forms), nullptr);
}

int fdsr_weights_complete(fdsr_handle h) {
  if (!h) return 0;
  for (const auto& w : h->weights)
    if (w.live && !w.loaded) return 0;
  return 1;
}

int fdsr_set_schedule(fdsr_handle h, const fdsr_schedule* s) {
  if (!h || !s || s->n_timestep < 1 || !s->noise_level || !s->sqrt_recip || !s->sqrt_recipm1 || !s->coef1 || !s->coef2 || !s->sigma)
    return fail(h, FDSR_E_INVALID, "bad schedule");
  h->T = s->n_timestep;
  auto cp = [&](std::vector<float>& v, const float* p) { v.assign(p, p + s->n_timestep); };
  cp(h->s_nl, s->noise_level); cp(h->s_recip, s->sqrt_recip); cp(h->s_recipm1, s->sqrt_recipm1);
  cp(h->s_c1, s->coef1); cp(h->s_c2, s->coef2); cp(h->s_sigma, s->sigma);
  return apply_plan(h, fdsr_forms::on_schedule(h->forms), nullptr);
}

int fdsr_workspace_bytes(fdsr_handle h, int batch, int height, int width, size_t* bytes) {
  if (!h || !bytes) return fail(h, FDSR_E_INVALID, "null argument");
  ShapePlan sp;
  int rc = make_shape_plan(h, batch, height, width, &sp);
  if (rc) return rc;
  *bytes = sp.bytes;
  return FDSR_OK;
}

int fdsr_unet_forward(fdsr_handle h, const float* x_nchw, const float* noise_level, float* eps_nchw, int batch, int height,
                      int width, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!h || !x_nchw || !noise_level || !eps_nchw) return fail(h, FDSR_E_INVALID, "null argument");
  int rc = plan_ready(h, false, batch, height, width, workspace, workspace_bytes);
  if (rc) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  char* ws = reinterpret_cast<char*>(workspace);
  float* xin = reinterpret_cast<float*>(ws + h->plan.tensor_off[h->t_in]);
  if ((rc = apply_plan(h, fdsr_forms::need_forward(h->forms, h->prec, h->training), st))) return rc;
  if (h->prec == PREC_F16X3 && g_tun.sat_guard) HIPCHK(h, hipMemsetAsync(h->d_sat, 0, sizeof(int), st));
  HIPCHK(h, launch_nchw_to_nhwc(x_nchw, xin, batch, h->cfg.in_channel, height, width, h->CP, 0, 1, st));
  if ((rc = run_unet(h, batch, height, width, ws, noise_level, 0.f, st))) return rc;
  const float* eps = reinterpret_cast<const float*>(ws + h->plan.tensor_off[h->t_eps]);
  HIPCHK(h, launch_nhwc_to_nchw(eps, eps_nchw, batch, h->cfg.out_channel, height, width, h->cfg.out_channel, st));
  return FDSR_OK;
}

int fdsr_tensor2img_u8(fdsr_handle h, const float* src_nchw, uint8_t* dst_nhwc, int batch, int channels, int height, int width,
                       float lo, float hi, void* hip_stream) {
  if (!src_nchw || !dst_nhwc || batch < 1 || channels < 1 || height < 1 || width < 1 || !(hi > lo))
    return fail(h, FDSR_E_INVALID, "bad tensor2img arguments");
  HIPCHK(h, launch_tensor2img_u8(src_nchw, dst_nhwc, batch, channels, height, width, lo, hi, reinterpret_cast<hipStream_t>(hip_stream)));
  return FDSR_OK;
}

int fdsr_u8_to_tensor(fdsr_handle h, const uint8_t* src_nhwc, float* dst_nchw, int batch, int channels, int height, int width,
                      float lo, float hi, void* hip_stream) {
  if (!src_nhwc || !dst_nchw || batch < 1 || channels < 1 || height < 1 || width < 1 || !(hi > lo))
    return fail(h, FDSR_E_INVALID, "bad u8_to_tensor arguments");
  HIPCHK(h, launch_u8_to_tensor(src_nhwc, dst_nchw, batch, channels, height, width, lo, hi, reinterpret_cast<hipStream_t>(hip_stream)));
  return FDSR_OK;
}

int fdsr_image_metrics_workspace_bytes(int batch, int height, int width, size_t* bytes) {
  if (!bytes || batch < 1 || height < 1 || width < 1) return fail(nullptr, FDSR_E_INVALID, "bad image-metrics shape");
  *bytes = image_metrics_workspace_bytes(batch, height, width);
  return FDSR_OK;
}

int fdsr_image_metrics_u8(fdsr_handle h, const uint8_t* test_nhwc, const uint8_t* truth_nhwc, int batch, int height, int width,
                          int channels, int flags, double* out_dev, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (!test_nhwc || !truth_nhwc || !out_dev || !workspace || batch < 1 || channels < 1 || channels > 4 ||
      !(flags & (FDSR_SSIM_UNIFORM7 | FDSR_SSIM_GAUSS11)) || (flags & ~(FDSR_SSIM_UNIFORM7 | FDSR_SSIM_GAUSS11)))
    return fail(h, FDSR_E_INVALID, "bad image-metrics arguments (1..4 channels; flags = FDSR_SSIM_UNIFORM7 | FDSR_SSIM_GAUSS11)");
  const int need = (flags & FDSR_SSIM_GAUSS11) ? 11 : 7;       // skimage raises for images smaller than the window too
  if (height < need || width < need) return fail(h, FDSR_E_INVALID, "image smaller than the %dx%d SSIM window", need, need);
  if (workspace_bytes < image_metrics_workspace_bytes(batch, height, width) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return fail(h, FDSR_E_WORKSPACE, "image-metrics workspace too small or misaligned");
  HIPCHK(h, launch_image_metrics_u8(test_nhwc, truth_nhwc, batch, height, width, channels, flags, out_dev, workspace,
                                    reinterpret_cast<hipStream_t>(hip_stream)));
  return FDSR_OK;
}

namespace {
// Pillow libImaging/Resample.c: bicubic_filter (a = -0.5), precompute_coeffs, normalize_coeffs_8bpc
double pil_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
struct ResizeTable { int in_size, out_size, ksize; int* d_bounds; int* d_kk; };
std::vector<ResizeTable> g_resize_tables;

int get_resize_table(fdsr_handle h, int in_size, int out_size, ResizeTable* out) {
  for (const auto& t : g_resize_tables)
    if (t.in_size == in_size && t.out_size == out_size) { *out = t; return FDSR_OK; }
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  const double ss = 1.0 / filterscale;
  std::vector<int> bounds((size_t)out_size * 2), kk((size_t)out_size * ksize, 0);
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) { w[x] = pil_bicubic((x + xmin - center + 0.5) * ss); ww += w[x]; }
    for (int x = 0; x < xmax; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (double)(1 << 22)) : (int)(0.5 + v * (double)(1 << 22));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  ResizeTable t{in_size, out_size, ksize, nullptr, nullptr};
  HIPCHK(h, hipMalloc((void**)&t.d_bounds, bounds.size() * sizeof(int)));
  HIPCHK(h, hipMalloc((void**)&t.d_kk, kk.size() * sizeof(int)));
  HIPCHK(h, hipMemcpy(t.d_bounds, bounds.data(), bounds.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(t.d_kk, kk.data(), kk.size() * sizeof(int), hipMemcpyHostToDevice));
  g_resize_tables.push_back(t);
  *out = t;
  return FDSR_OK;
}
}  // namespace

int fdsr_resize_bicubic_u8(fdsr_handle h, const uint8_t* src_nhwc, int batch, int in_h, int in_w, int out_h, int out_w,
                           uint8_t* tmp, uint8_t* dst_u8_nhwc, float* dst_f32_nchw, void* hip_stream) {
  if (!src_nhwc || !tmp || (!dst_u8_nhwc && !dst_f32_nchw) || batch < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1)
    return fail(h, FDSR_E_INVALID, "bad resize arguments");
  ResizeTable tx{}, ty{};
  int rc = get_resize_table(h, in_w, out_w, &tx);
  if (rc) return rc;
  if ((rc = get_resize_table(h, in_h, out_h, &ty))) return rc;
  HIPCHK(h, launch_resize_bicubic_u8(src_nhwc, tmp, dst_u8_nhwc, dst_f32_nchw, batch, in_h, in_w, out_h, out_w, tx.d_bounds, tx.d_kk,
                                     tx.ksize, ty.d_bounds, ty.d_kk, ty.ksize, reinterpret_cast<hipStream_t>(hip_stream)));
  return FDSR_OK;
}

int fdsr_set_precision(fdsr_handle h, int mode) {
  if (!h || mode < 0 || mode > PREC_F16) return fail(h, FDSR_E_INVALID, "precision mode must be 0 (f32), 1 (f16x3), 2 (bf16) or 3 (f16)");
  if (prec_is16(mode)) {
    // bf16 / f16 mode stores activations in 16 bits: every conv but the packed-input one must run on the 16-bit
    // kernels (attention and the GDP resampling kernels have bf16 forms of their own)
    for (const Op& op : h->ops) {
      if (op.kind == Op::CONV && !h->weights[op.w].h_ok && op.src0 != h->t_in)
        return fail(h, FDSR_E_INVALID, "the 16-bit storage modes need channel counts that are multiples of 16 (layer %s)", op.name.c_str());
    }
  }
  int rc = apply_plan(h, fdsr_forms::on_precision(h->forms, h->prec, mode), nullptr);
  if (rc) return rc;
  h->prec = mode;
  return FDSR_OK;
}

int fdsr_set_dropout_seed(fdsr_handle h, uint64_t seed) {
  if (!h) return FDSR_E_INVALID;
  h->drop_seed = seed;
  h->drop_step = 0;
  return FDSR_OK;
}

int fdsr_set_training(fdsr_handle h, int on) {
  if (!h) return FDSR_E_INVALID;
  if (on && h->cfg.dropout >= 1.0f) return fail(h, FDSR_E_INVALID, "dropout must be < 1");
  h->training = on != 0;
  return FDSR_OK;
}

int fdsr_debug_dropout_mask(fdsr_handle h, const char* block, const unsigned char** dev_off, int* n, int* hgt, int* wid, int* ch,
                            float* scale) {
  if (!h || !block) return fail(h, FDSR_E_INVALID, "null argument");
  if (!h->plan.bytes || !h->plan.training) return fail(h, FDSR_E_STATE, "no training-mode forward has run yet");
  const std::string want = std::string(block) + ".res_block.block2";
  for (const Op& op : h->ops)
    if (op.kind == Op::CONV && op.drop_slot >= 0 && op.name == want) {
      if (dev_off) *dev_off = reinterpret_cast<const unsigned char*>(h->plan.drop_off[op.drop_slot]);   // offset into the workspace
      if (n) *n = h->plan.N;
      if (hgt) *hgt = h->plan.H >> op.lvl_in;
      if (wid) *wid = h->plan.W >> op.lvl_in;
      if (ch) *ch = op.C0;
      if (scale) *scale = 1.0f / (1.0f - h->cfg.dropout);
      return FDSR_OK;
    }
  return fail(h, FDSR_E_KEY, "no dropout in front of block '%s'", block);
}

int fdsr_check_saturation(fdsr_handle h, void* hip_stream) {
  if (!h) return FDSR_E_INVALID;
  if (!h->d_sat) return FDSR_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  if (!h->h_sat) HIPCHK(h, hipHostMalloc((void**)&h->h_sat, 64, hipHostMallocDefault));   // pinned: the copy below is truly asynchronous
  *h->h_sat = 0;
  HIPCHK(h, hipMemcpyAsync(h->h_sat, h->d_sat, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (!*h->h_sat) return FDSR_OK;
  HIPCHK(h, hipMemsetAsync(h->d_sat, 0, sizeof(int), st));
  return fail(h, FDSR_E_SATURATED, "f16x3: a raw convolution input exceeded the f16 range (+-65504) and was clamped; "
                                   "re-run this call with fdsr_set_precision(FDSR_PREC_F32)");
}

int fdsr_debug_option(const char* name, long long value) {
  return set_tunable(name, value) == 0 ? FDSR_OK : FDSR_E_INVALID;
}

int fdsr_set_debug(fdsr_handle h, int on) {
  if (!h) return FDSR_E_INVALID;
  h->debug = on != 0;
  return FDSR_OK;
}

int fdsr_debug_tensor(fdsr_handle h, const char* name, const float** dev_ptr, int* n, int* hgt, int* wid, int* ch) {
  if (!h || !name) return fail(h, FDSR_E_INVALID, "null argument");
  if (!h->plan.bytes) return fail(h, FDSR_E_STATE, "no forward has run yet");
  for (size_t t = 0; t < h->tensors.size(); ++t)
    if (h->tensors[t].name == name) {
      if (dev_ptr) *dev_ptr = reinterpret_cast<const float*>(h->plan.tensor_off[t]);   // offset; caller adds the workspace base
      if (n) *n = h->plan.N;
      if (hgt) *hgt = h->plan.H >> h->tensors[t].level;
      if (wid) *wid = h->plan.W >> h->tensors[t].level;
      if (ch) *ch = h->tensors[t].C;
      return FDSR_OK;
    }
  return fail(h, FDSR_E_KEY, "no tensor named '%s'", name);
}

int fdsr_debug_gn_table(fdsr_handle h, const char* conv, const float** dev_ptr, int* n, int* ch) {
  if (!h || !conv) return fail(h, FDSR_E_INVALID, "null argument");
  if (!h->plan.bytes) return fail(h, FDSR_E_STATE, "no forward has run yet");
  for (const Op& op : h->ops)
    if (op.kind == Op::CONV && op.gn_slot >= 0 && op.name == conv) {
      if (dev_ptr) *dev_ptr = reinterpret_cast<const float*>(h->plan.gn_off[op.gn_slot]);   // offset; caller adds the workspace base
      if (n) *n = h->plan.N;
      if (ch) *ch = op.C0 + op.C1;
      return FDSR_OK;
    }
  return fail(h, FDSR_E_KEY, "no GroupNorm'ed convolution named '%s'", conv);
}

int fdsr_debug_tensor_elem_bytes(fdsr_handle h, const char* name, int* bytes) {
  if (!h || !name || !bytes) return fail(h, FDSR_E_INVALID, "null argument");
  for (size_t t = 0; t < h->tensors.size(); ++t)
    if (h->tensors[t].name == name) {
      *bytes = (prec_is16(h->prec) && (int)t != h->t_in && (int)t != h->t_eps) ? 2 : 4;
      return FDSR_OK;
    }
  return fail(h, FDSR_E_KEY, "no tensor named '%s'", name);
}

int fdsr_profile_begin(fdsr_handle h) {
  if (!h) return FDSR_E_INVALID;
  h->profiling = true;
  h->prof_step = true;
  h->ev_used = 0;
  h->prof_flops = h->prof_bytes = 0;
  return FDSR_OK;
}

int fdsr_profile_end(fdsr_handle h, int* launches, double* conv_ms, double* conv_flops_out, double* conv_bytes) {
  if (!h) return FDSR_E_INVALID;
  h->profiling = false;
  double ms = 0;
  if (h->ev_used) HIPCHK(h, hipEventSynchronize(h->ev_pool[h->ev_used - 1]));
  for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
    float m = 0;
    HIPCHK(h, hipEventElapsedTime(&m, h->ev_pool[i], h->ev_pool[i + 1]));
    ms += m;
  }
  if (launches) *launches = (int)(h->ev_used / 2);
  if (conv_ms) *conv_ms = ms;
  if (conv_flops_out) *conv_flops_out = h->prof_flops;
  if (conv_bytes) *conv_bytes = h->prof_bytes;
  h->ev_used = 0;
  return FDSR_OK;
}

}  // extern "C"
