// Which device forms of the UNet's weights follow the fp32 master copy (fdsr_engine::d_master), and who packed them.
// One record per engine; the rules live in fdsr_forms.cpp.  Nothing here touches the device: events and reader
// requirements return the packing passes to run, apply_plan() (fdsr_engine_int.h) runs them and reports each back
// through done().  DESIGN.md section 11 has the table of family x event x packer.
#pragma once
#include <cstdint>

namespace fdsr_forms {

enum Family {
  FWD32,    // fp32 forward packs in d_params, and the table-copied small tensors
  WT32,     // transposed fp32 forms in d_wt
  FWD_H3,   // f16x3 forward fragments with their d_hscale pair (the f16 mode reads their hi plane)
  UP2_H3,   // f16x3 sub-pixel form of the upsample convs: HOST = scale in WeightEntry::up2_inv_scale, DEVICE = scale in d_up2_inv
  B16,      // bf16 forward and sub-pixel forms (the host packs them, nobody else)
  WT_H3,    // transposed f16x3 fragments in d_wtq
  TEMB,     // the [T][TE] embedding table
  SCHED,    // device copy of the posterior scalars (fdsr_sample_stepwise)
  N_FAMILY
};

// BEHIND: lags the master copy (or, for UP2_H3, no longer has ONE scale source).  LAZY (FWD32 only): f16x3 optimiser steps
// refreshed just the members they read themselves; the fp32 conv forms with an f16x3 twin, d_wt slots included, lag.
enum Src : uint8_t { BEHIND, LAZY, HOST, DEVICE };

enum Pass : uint8_t {
  DEVICE_SYNC,      // hipDeviceSynchronize
  SYNC16,           // hipDeviceSynchronize, then the host re-packs every 16-bit forward form (fdsr_sync_weight_forms)
  PACK_T,           // device: d_wt, d_hscale, d_wtq
  PACK_STEP_LAZY,   // device, f16x3 step: the fp32 forms without a twin, d_hscale, f16x3 forward + sub-pixel, d_wtq
  PACK_STEP_FULL,   // device, step in another mode: every fp32 form too
  PACK_ALL32,       // as PACK_STEP_FULL, asked for by a switch to fp32 (clears LAZY)
  TEMB_TABLE,
  STEP_SCHED
};

enum { F32 = 0, F16X3 = 1, BF16 = 2, F16 = 3 };                     // enum Precision (fdsr_kernels.h)
enum Up2 { UP2_GENERIC, UP2_HOST_SCALE, UP2_DEVICE_SCALE };         // the upsample conv: generic kernel, or sub-pixel fragments + scale source

struct Forms {
  Src st[N_FAMILY] = {HOST, BEHIND, HOST, HOST, HOST, BEHIND, BEHIND, BEHIND};   // every weight loaded (the host packs at load), nothing else made yet
  bool lazy_skips = false;   // some conv has f16x3 forms: a lazy step leaves fp32 forms behind (false until training is prepared)
};

struct Plan {
  int n = 0;
  Pass pass[4] = {};
  bool drop_captures = false;   // the captured sampling graphs bake what this event changed
};

// events
Plan on_load(Forms& f);                     // one tensor loaded: the host packed its forward forms
Plan on_schedule(Forms& f);
Plan on_step(const Forms& f, int prec);     // optimiser step: lazy in f16x3 mode, full otherwise
Plan on_precision(const Forms& f, int from, int to);
Plan on_sync(const Forms& f);               // fdsr_sync_weight_forms
// readers
Plan need_forward(const Forms& f, int prec, bool training);     // fdsr_unet_forward
Plan need_sample(const Forms& f, int prec, bool stepwise);      // fdsr_sample / fdsr_sample_stepwise: eval-mode forms, table, (schedule copy)
Plan need_train(const Forms& f, int prec);                      // the training step
Up2 up2_form(const Forms& f, int prec);                         // run_unet, a 16-bit upsample conv
void done(Forms& f, Pass p);                                    // pass p ran

}  // namespace fdsr_forms
