// The device forms of the UNet's weights: the record of which follow the master copy (fdsr_forms.h: rules without a device,
// driven by tests/test_weight_forms_host.py), the one function that runs the packing passes the record asks for, and the
// host side of packing itself (checkpoint repack at load, layout of the transposed arenas, device re-pack from the master copy).
#include "fdsr_forms.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "fdsr_engine_int.h"
#include "fdsr_train.h"

using namespace fdsr;
using namespace fdsr_int;

// ---- the record ------------------------------------------------------------------------------------------------------------
// A family is read in EVAL mode (sampling, an eval forward, a switch of the precision) only as the host packed it: a fresh engine
// loaded with the same weights then computes the same bits (the two packers round the sub-pixel forms differently).  TRAINING
// mode (the step, a train-mode forward) reads whatever follows the master copy.
namespace fdsr_forms {
static_assert(F32 == PREC_F32 && F16X3 == PREC_F16X3 && BF16 == PREC_BF16 && F16 == PREC_F16, "precision codes");

static void add(Plan& p, Pass x) { p.pass[p.n++] = x; }

Plan on_load(Forms& f) {
  f.st[WT32] = f.st[WT_H3] = BEHIND;
  if (f.st[UP2_H3] == DEVICE) f.st[UP2_H3] = BEHIND;   // this tensor's sub-pixel form carries the host's scale again: two scale sources
  f.st[TEMB] = BEHIND;
  Plan p;
  p.drop_captures = true;   // weights are baked by address only, but be safe
  return p;
}

Plan on_schedule(Forms& f) {
  f.st[TEMB] = f.st[SCHED] = BEHIND;
  Plan p;
  p.drop_captures = true;
  return p;
}

// In f16x3 mode a step reads the fp32 conv forms only where the 16-bit kernels cannot run (the packed-input conv, odd shapes):
// the others wait until something asks for them (on_precision).
Plan on_step(const Forms&, int prec) {
  Plan p;
  add(p, prec == F16X3 ? PACK_STEP_LAZY : PACK_STEP_FULL);
  p.drop_captures = true;
  return p;
}

Plan need_forward(const Forms& f, int prec, bool training) {
  Plan p;
  const int wform = prec == F16 ? F16X3 : prec;   // prec_wform
  if (wform == F16X3 && !training && (f.st[FWD_H3] != HOST || f.st[UP2_H3] != HOST)) add(p, SYNC16);
  if (wform == BF16 && f.st[B16] == BEHIND) add(p, SYNC16);   // in training mode too: only the host packs bf16
  return p;
}

// The 16-bit forms that lag behind optimiser steps are refreshed when the mode is SWITCHED to and by the calls that read them in
// eval mode -- not when a training loop merely re-states its precision before every step (a host re-pack of every weight per step).
Plan on_precision(const Forms& f, int from, int to) {
  Plan p;
  if (to == F32 && f.st[FWD32] == LAZY) {
    // the optimiser step that left them behind may still be queued on a non-blocking stream the NULL stream does not order after
    add(p, DEVICE_SYNC); add(p, PACK_ALL32); add(p, DEVICE_SYNC);
  } else if (to != F32 && to != from) {
    p = need_forward(f, to, false);
  }
  p.drop_captures = from != to;
  return p;
}

Plan on_sync(const Forms& f) {
  Plan p;
  if (f.st[B16] == BEHIND || f.st[FWD_H3] != HOST || f.st[UP2_H3] != HOST) add(p, SYNC16);
  return p;
}

Plan need_sample(const Forms& f, int prec, bool stepwise) {
  const bool sync = need_forward(f, prec, false).n > 0;
  Plan p;
  if (stepwise && sync) add(p, SYNC16);
  if (f.st[TEMB] == BEHIND) add(p, TEMB_TABLE);
  if (!stepwise && sync) add(p, SYNC16);
  if (stepwise && f.st[SCHED] == BEHIND) add(p, STEP_SCHED);
  return p;
}

// f16x3: the forward forms are re-packed on the device here too, as every optimiser step will: a run resumed from a checkpoint
// (host-packed at load) then steps on the same bits as the uninterrupted run.
Plan need_train(const Forms& f, int prec) {
  Plan p;
  if (prec == F32 && f.st[FWD32] == LAZY) add(p, PACK_ALL32);
  if (f.st[WT32] == BEHIND || f.st[WT_H3] == BEHIND) add(p, prec == F16X3 ? PACK_STEP_LAZY : PACK_T);
  return p;
}

Up2 up2_form(const Forms& f, int prec) {
  if (prec == BF16) return f.st[B16] == BEHIND ? UP2_GENERIC : UP2_HOST_SCALE;
  return f.st[UP2_H3] == DEVICE ? UP2_DEVICE_SCALE : (f.st[UP2_H3] == HOST ? UP2_HOST_SCALE : UP2_GENERIC);
}

void done(Forms& f, Pass p) {
  switch (p) {
    case DEVICE_SYNC: return;
    case SYNC16: f.st[FWD_H3] = f.st[UP2_H3] = f.st[B16] = HOST; return;
    case TEMB_TABLE: f.st[TEMB] = DEVICE; return;
    case STEP_SCHED: f.st[SCHED] = HOST; return;
    default: break;
  }
  f.st[TEMB] = BEHIND;   // the table is evaluated from d_params
  if (p != PACK_T) {
    f.st[FWD_H3] = f.st[UP2_H3] = DEVICE;
    f.st[B16] = BEHIND;
  }
  // Two rules kept from before the record, each worth one redundant pass: PACK_ALL32 writes d_wt and d_wtq but leaves their
  // state alone (a load before the switch still costs PACK_T at the next step), and a full step leaves LAZY standing.
  if (p != PACK_ALL32) f.st[WT32] = f.st[WT_H3] = DEVICE;
  if (p == PACK_ALL32) f.st[FWD32] = DEVICE;
  else if (p == PACK_STEP_LAZY && f.lazy_skips) f.st[FWD32] = LAZY;
  else if (p == PACK_STEP_FULL && f.st[FWD32] != LAZY) f.st[FWD32] = DEVICE;
}

}  // namespace fdsr_forms

using namespace fdsr_forms;

// ---- host packing at load --------------------------------------------------------------------------------------------------
namespace {

inline uint16_t f32_to_bf16_rn(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

inline uint16_t f32_to_f16_rn(float f) {
  _Float16 hv = (_Float16)f;
  uint16_t b;
  memcpy(&b, &hv, 2);
  return b;
}

// Repack a Conv2d weight [Cout][Cin][ks][ks] into MFMA B-fragment order for the 16-bit kernels:
// [cot][kc][wn][tap][plane][lane] x 8 halves, element j of lane l = W[co = cot*BN + wn*32 + (l&31)]
// [k = kc*16 + 8*(l>>5) + j][tap]   (v_mfma_f32_32x32x16 B operand map).
// f16x3: plane 0 = hi = f16(w*s), plane 1 = lo = f16(w*s - hi), s = 2^e chosen so that max|w*s| < 2^15
// (keeps lo out of the f16 subnormal range for all but tiny weights); bf16: one plane, s = 1.
int pack_weights_h(fdsr_handle h, WeightEntry& w, const float* host) {
  const int Cout = (int)w.shape[0], Cin = (int)w.shape[1], ks = w.ks, T = ks * ks;
  const int WN = w.h_WN, BN = 32 * WN, ncot = w.h_cout_pad / BN, nk = w.h_cin_pad / 16;
  float amax = 0.f;
  for (size_t i = 0; i < numel(w.shape); ++i) amax = std::max(amax, std::fabs(host[i]));
  int e = 12;
  if (amax > 0.f) e = std::min(12, (int)std::floor(std::log2(32768.0 / (double)amax)));
  const float scale = std::ldexp(1.0f, e);
  w.h_inv_scale[PREC_F16X3] = std::ldexp(1.0f, -e);
  w.h_inv_scale[PREC_BF16] = 1.0f;
  const size_t nfrag = (size_t)ncot * nk * WN * T * 64;   // 16-byte fragments per plane set
  std::vector<uint16_t> q3(nfrag * 2 * 8, 0), qb(nfrag * 8, 0);
  for (int cot = 0; cot < ncot; ++cot)
    for (int kc = 0; kc < nk; ++kc)
      for (int wn = 0; wn < WN; ++wn)
        for (int t = 0; t < T; ++t)
          for (int l = 0; l < 64; ++l) {
            const int co = cot * BN + wn * 32 + (l & 31);
            const size_t f3 = (((((size_t)cot * nk + kc) * WN + wn) * T + t) * 2) * 64 + l;
            const size_t fb = (((((size_t)cot * nk + kc) * WN + wn) * T + t) * 1) * 64 + l;
            for (int j = 0; j < 8; ++j) {
              const int k = kc * 16 + 8 * (l >> 5) + j;
              float v = 0.f;
              if (co < Cout && k < Cin) v = host[((size_t)co * Cin + k) * T + t];
              const float vs = v * scale;
              const uint16_t hi = f32_to_f16_rn(vs);
              _Float16 hif;
              memcpy(&hif, &hi, 2);
              const uint16_t lo = f32_to_f16_rn(vs - (float)hif);
              q3[f3 * 8 + j] = hi;
              q3[(f3 + 64) * 8 + j] = lo;
              qb[fb * 8 + j] = f32_to_bf16_rn(v);
            }
          }
  {
    const float sc2[2] = {scale, w.h_inv_scale[PREC_F16X3]};
    const size_t widx = (size_t)(&w - h->weights.data());
    HIPCHK(h, hipMemcpy(h->d_hscale + 2 * widx, sc2, sizeof sc2, hipMemcpyHostToDevice));
  }
  HIPCHK(h, hipMemcpy(h->d_wq + w.hq_off[PREC_F16X3], q3.data(), q3.size() * 2, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_wq + w.hq_off[PREC_BF16], qb.data(), qb.size() * 2, hipMemcpyHostToDevice));
  if (w.ck != CONV3_UP) return FDSR_OK;

  // Sub-pixel form of Upsample(nearest x2)+Conv3x3 (unet.py:66-74): W2[py][px][a][b] = sum of the 3x3 taps
  // that land on source offset (a, b) for output parity (py, px); R(0,0)={0} R(0,1)={1,2} R(1,0)={0,1} R(1,1)={2}.
  auto tapset = [](int par, int a, int* lo, int* hi) {
    if (par == 0) { if (a == 0) { *lo = 0; *hi = 0; } else { *lo = 1; *hi = 2; } }
    else          { if (a == 0) { *lo = 0; *hi = 1; } else { *lo = 2; *hi = 2; } }
  };
  std::vector<float> w2((size_t)Cout * Cin * 16, 0.f);   // [co][ci][py][px][a][b]
  float amax2 = 0.f;
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
          for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
              int y0, y1, x0, x1;
              tapset(py, a, &y0, &y1);
              tapset(px, b, &x0, &x1);
              float acc = 0.f;
              for (int ky = y0; ky <= y1; ++ky)
                for (int kx = x0; kx <= x1; ++kx) acc += host[((size_t)co * Cin + ci) * 9 + ky * 3 + kx];
              w2[((size_t)co * Cin + ci) * 16 + ((py * 2 + px) * 2 + a) * 2 + b] = acc;
              amax2 = std::max(amax2, std::fabs(acc));
            }
  int e2 = 12;
  if (amax2 > 0.f) e2 = std::min(12, (int)std::floor(std::log2(32768.0 / (double)amax2)));
  const float scale2 = std::ldexp(1.0f, e2);
  w.up2_inv_scale[PREC_F16X3] = std::ldexp(1.0f, -e2);
  w.up2_inv_scale[PREC_BF16] = 1.0f;
  const size_t nfrag2 = (size_t)ncot * nk * WN * 16 * 64;
  std::vector<uint16_t> u3(nfrag2 * 2 * 8, 0), ub(nfrag2 * 8, 0);
  for (int cot = 0; cot < ncot; ++cot)
    for (int kc = 0; kc < nk; ++kc)
      for (int wn = 0; wn < WN; ++wn)
        for (int py = 0; py < 2; ++py)
          for (int slot = 0; slot < 8; ++slot)
            for (int l = 0; l < 64; ++l) {
              const int px = slot >> 2, a = (slot >> 1) & 1, b = slot & 1;
              const int co = cot * BN + wn * 32 + (l & 31);
              const size_t fidx = ((((size_t)cot * nk + kc) * WN + wn) * 2 + py) * 8 + slot;
              for (int j = 0; j < 8; ++j) {
                const int k = kc * 16 + 8 * (l >> 5) + j;
                float v = 0.f;
                if (co < Cout && k < Cin) v = w2[((size_t)co * Cin + k) * 16 + ((py * 2 + px) * 2 + a) * 2 + b];
                const float vs = v * scale2;
                const uint16_t hi = f32_to_f16_rn(vs);
                _Float16 hif;
                memcpy(&hif, &hi, 2);
                u3[((fidx * 2 + 0) * 64 + l) * 8 + j] = hi;
                u3[((fidx * 2 + 1) * 64 + l) * 8 + j] = f32_to_f16_rn(vs - (float)hif);
                ub[(fidx * 64 + l) * 8 + j] = f32_to_bf16_rn(v);
              }
            }
  HIPCHK(h, hipMemcpy(h->d_wq + w.up2_off[PREC_F16X3], u3.data(), u3.size() * 2, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->d_wq + w.up2_off[PREC_BF16], ub.data(), ub.size() * 2, hipMemcpyHostToDevice));
  return FDSR_OK;
}

// SYNC16: every 16-bit forward form from the master copy, through the packer of the load path
int host_pack16(fdsr_handle h) {
  HIPCHK(h, hipDeviceSynchronize());
  std::vector<float> host;
  for (int i = 0; i < h->n_schema; ++i) {
    WeightEntry& w = h->weights[i];
    if (!w.live || w.sink != WeightEntry::CONV_PACK || !w.h_ok) continue;
    host.resize(numel(w.shape));
    HIPCHK(h, hipMemcpy(host.data(), h->d_master + h->master_off[i], host.size() * sizeof(float), hipMemcpyDeviceToHost));
    int rc = pack_weights_h(h, w, host.data());
    if (rc) return rc;
  }
  return FDSR_OK;
}

// the device passes (PACK_T, PACK_STEP_LAZY, PACK_STEP_FULL, PACK_ALL32): every form they name, from the master copy
int repack_from_master(fdsr_handle h, hipStream_t st, Pass pass) {
  const bool forward_forms = pass != PACK_T, lazy = pass == PACK_STEP_LAZY;
  if (forward_forms) {
    for (int i = 0; i < h->n_schema; ++i) {
      WeightEntry& w = h->weights[i];
      if (!w.live || w.sink != WeightEntry::CONV_PACK || (lazy && w.h_ok)) continue;
      HIPCHK(h, launch_pack_conv_f32(h->d_master + h->master_off[i], h->d_params + w.dev_off, (int)w.shape[0], (int)w.shape[1], w.ks,
                                     w.cout_pad, w.cin_pad, st));
    }
    HIPCHK(h, launch_copy_table(h->d_master, h->d_params, h->d_copy_tab, h->n_copy_tab, st, h->copy_tab_max));
  }
  auto each_slot = [&](bool quantised, auto&& pack) -> hipError_t {   // the transposed slots of every conv that has an input gradient
    for (const Op& op : h->ops) {
      if (op.kind != Op::CONV || op.src0 == h->t_in) continue;
      const WtSlots& ws = h->wt_slots[op.w];
      const bool has_q = ws.s[0].wtq_off != SIZE_MAX;
      if (quantised ? !has_q : (lazy && has_q)) continue;   // a lazy step leaves the fp32 slot of a conv with f16x3 fragments behind
      const WeightEntry& w = h->weights[op.w];
      for (int i = 0; i < ws.n; ++i) {
        hipError_t e = pack(op, w, h->d_master + h->master_off[op.w], ws.s[i], t_dims(op.ck, conv_K(h, op), ws.s[i].rows));
        if (e != hipSuccess) return e;
      }
    }
    return hipSuccess;
  };
  HIPCHK(h, each_slot(false, [&](const Op&, const WeightEntry& w, const float* src, const WtSlot& s, const TDims& d) {
    return launch_pack_conv_f32_t(src, h->d_wt + s.wt_off, (int)w.shape[0], (int)w.shape[1], w.ks, s.c_off, s.rows, d.rows_pad, d.cols_pad, st);
  }));
  // f16x3 forms (forward + transposed), packed on the device with a per-tensor power-of-two scale
  HIPCHK(h, hipMemsetAsync(h->d_hamax, 0, h->weights.size() * sizeof(unsigned), st));
  for (int i = 0; i < h->n_schema; ++i) {
    const WeightEntry& w = h->weights[i];
    if (w.live && w.sink == WeightEntry::CONV_PACK && w.h_ok)
      HIPCHK(h, launch_hamax(h->d_master + h->master_off[i], numel(w.shape), h->d_hamax + i, st));
  }
  // every slot gets a scale; the slots that are not f16x3 conv weights (amax 0 -> e = 12) are never read
  HIPCHK(h, launch_hscale_all(h->d_hamax, h->d_hscale, (int)h->weights.size(), st));
  for (int i = 0; i < h->n_schema && forward_forms; ++i) {
    WeightEntry& w = h->weights[i];
    if (!w.live || w.sink != WeightEntry::CONV_PACK || !w.h_ok) continue;
    const float* src = h->d_master + h->master_off[i];
    float* sc2 = h->d_hscale + 2 * (size_t)i;
    HIPCHK(h, launch_pack_conv_h(src, h->d_wq + w.hq_off[PREC_F16X3], sc2, (int)w.shape[0], (int)w.shape[1], w.ks, w.h_WN,
                                 w.h_cout_pad, w.h_cin_pad, 0, 0, 0, st));
    if (w.ck == CONV3_UP)   // and the sub-pixel form the upsample convs run on
      HIPCHK(h, launch_pack_conv_up2_h(src, h->d_wq + w.up2_off[PREC_F16X3], sc2, h->d_up2_inv + i, (int)w.shape[0], (int)w.shape[1],
                                       w.h_WN, w.h_cout_pad, w.h_cin_pad, st));
  }
  HIPCHK(h, each_slot(true, [&](const Op& op, const WeightEntry& w, const float* src, const WtSlot& s, const TDims& d) {
    return launch_pack_conv_h(src, h->d_wtq + s.wtq_off, h->d_hscale + 2 * (size_t)op.w, (int)w.shape[0], (int)w.shape[1], w.ks, d.WN,
                              d.rows_pad_h, d.K_pad_h, 1, s.c_off, s.rows, st);
  }));
  return FDSR_OK;
}

}  // namespace

namespace fdsr_int {

TDims t_dims(ConvKind ck, int K, int rows) {
  const ConvKind k = ck == CONV1 ? CONV1 : CONV3_S1;     // the transposed conv always runs at stride 1
  int KC, BN, TH, WN;
  conv_tile_config(k, K, 0, rows, &KC, &BN);
  conv_h_config(k, rows, &TH, &WN);
  return TDims{round_up(rows, BN), round_up(K, KC), WN, round_up(rows, 32 * WN), round_up(K, 16)};
}

// the checkpoint tensor `host` of entry w into d_params, and into the 16-bit forward forms where w has them
int pack_weight_host(fdsr_handle h, WeightEntry& w, const float* host) {
  float* dst = h->d_params + w.dev_off;
  if (w.sink != WeightEntry::CONV_PACK) {
    HIPCHK(h, hipMemcpy(dst, host, numel(w.shape) * sizeof(float), hipMemcpyHostToDevice));
    return FDSR_OK;
  }
  const int Cout = (int)w.shape[0], Cin = (int)w.shape[1], ks = w.ks;
  std::vector<float> pk((size_t)ks * ks * w.cout_pad * w.cin_pad, 0.f);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int t = 0; t < ks * ks; ++t)
        pk[((size_t)t * w.cout_pad + co) * w.cin_pad + ci] = host[((size_t)co * Cin + ci) * ks * ks + t];
  HIPCHK(h, hipMemcpy(dst, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
  return w.h_ok ? pack_weights_h(h, w, host) : FDSR_OK;
}

// Layout and allocation of what the device passes write: per conv weight one transposed slot per concat source (a GroupNorm'ed
// input: one slot over all input channels) in d_wt, and the same as f16x3 MFMA fragments in d_wtq for the convs whose transposed
// shape the 16-bit kernels take (16-channel K chunks: K % 16 == 0 and the produced channel count % 16 == 0).
int prepare_train_forms(fdsr_handle h) {
  h->wt_slots.assign(h->weights.size(), WtSlots{});
  size_t off = 0, qoff = 0;
  for (const Op& op : h->ops) {
    if (op.kind != Op::CONV || op.src0 == h->t_in) continue;
    const int T = op.ck == CONV1 ? 1 : 9, K = conv_K(h, op);
    const bool whole = op.gn_slot >= 0 || op.C1 == 0, quantised = !(K % 16 || op.C0 % 16 || op.C1 % 16);
    WtSlots& ws = h->wt_slots[op.w];
    ws.n = whole ? 1 : 2;
    ws.s[0] = WtSlot{0, whole ? op.C0 + op.C1 : op.C0};
    ws.s[1] = WtSlot{op.C0, op.C1};
    for (int i = 0; i < ws.n; ++i) {
      const TDims d = t_dims(op.ck, K, ws.s[i].rows);
      ws.s[i].wt_off = off;
      off += align_up((size_t)T * d.rows_pad * d.cols_pad, 64);
      if (!quantised) continue;
      ws.s[i].wtq_off = qoff;
      qoff += align_up((size_t)(d.rows_pad_h / 32) * (d.K_pad_h / 16) * T * 64 * 16 * 2, 256);
      h->forms.lazy_skips = true;
    }
  }
  h->wt_floats = off;
  h->wtq_bytes = qoff;
  HIPCHK(h, hipMalloc((void**)&h->d_wtq, std::max<size_t>(qoff, 256)));
  HIPCHK(h, hipMalloc((void**)&h->d_hamax, h->weights.size() * sizeof(unsigned)));
  HIPCHK(h, hipMalloc((void**)&h->d_up2_inv, h->weights.size() * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->d_wt, std::max<size_t>(off, 4) * sizeof(float)));
  // the non-conv tensors (GroupNorm affine, biases, MLPs ...) follow the master copy through ONE table-driven copy
  std::vector<unsigned long long> tab;
  for (int i = 0; i < h->n_schema; ++i) {
    const WeightEntry& w = h->weights[i];
    if (!w.live) continue;
    if (w.sink == WeightEntry::CONV_PACK) { h->forms.lazy_skips |= w.h_ok; continue; }
    tab.push_back(h->master_off[i]);
    tab.push_back(w.dev_off);
    tab.push_back(numel(w.shape));
    h->copy_tab_max = std::max<size_t>(h->copy_tab_max, numel(w.shape));
  }
  h->n_copy_tab = (int)(tab.size() / 3);
  HIPCHK(h, hipMalloc((void**)&h->d_copy_tab, std::max<size_t>(tab.size(), 3) * sizeof(unsigned long long)));
  if (!tab.empty()) HIPCHK(h, hipMemcpy(h->d_copy_tab, tab.data(), tab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
  return FDSR_OK;
}

int apply_plan(fdsr_handle h, const Plan& p, hipStream_t st) {
  for (int i = 0; i < p.n; ++i) {
    int rc = FDSR_OK;
    switch (p.pass[i]) {
      case DEVICE_SYNC: HIPCHK(h, hipDeviceSynchronize()); break;
      case SYNC16: rc = host_pack16(h); break;
      case TEMB_TABLE: rc = build_temb_table(h, st); break;
      case STEP_SCHED: rc = upload_step_sched(h); break;
      default: rc = repack_from_master(h, st, p.pass[i]);
    }
    if (rc) return rc;
    done(h->forms, p.pass[i]);
  }
  if (p.drop_captures) drop_captures(h);
  return FDSR_OK;
}

}  // namespace fdsr_int

// Bring the 16-bit weight forms (f16x3 / bf16 sampling) in line with the master copy after optimiser steps.
extern "C" int fdsr_sync_weight_forms(fdsr_handle h) {
  if (!h) return FDSR_E_INVALID;
  return apply_plan(h, on_sync(h->forms), nullptr);
}
