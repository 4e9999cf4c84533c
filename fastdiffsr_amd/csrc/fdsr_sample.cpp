// The reverse-diffusion loop of libfdsr_hip.so: fdsr_sample (per-step inputs as kernel arguments, the whole loop as one graph) and
// fdsr_sample_stepwise (per-step inputs on the device, chunks of steps as graphs) run one head, one step and one loop; the captured
// graphs of both, the embedding table and the step state they read, and the engine's noise generator.  The UNet itself is
// run_unet (fdsr_engine.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "fdsr_engine_int.h"

using namespace fdsr;
using namespace fdsr_int;

namespace fdsr_int {

int fill_temb(fdsr_handle h, float* temb, int N, const float* nl_dev, float nl_scalar, hipStream_t st) {
  auto P = [&](int widx) -> const float* { return widx >= 0 ? h->d_params + h->weights[widx].dev_off : nullptr; };
  TembParams tp;
  tp.freq = P(h->w_freq);
  tp.w1 = P(h->w_mlp[0]);
  tp.b1 = P(h->w_mlp[1]);
  tp.w2 = P(h->w_mlp[2]);
  tp.b2 = P(h->w_mlp[3]);
  tp.wn = h->d_params + h->noise_w_off;   // all 22 noise_func Linear layers, concatenated by rows
  tp.bn = h->d_params + h->noise_b_off;
  tp.nl_dev = nl_dev;
  tp.nl_scalar = nl_scalar;
  tp.temb = temb;
  tp.inner = h->cfg.inner_channel;
  tp.TE = h->TE;
  tp.N = N;
  tp.swish_block = (h->sr3 || h->gdp) ? 1 : 0;
  tp.enc_dim = tp.hid_dim = tp.t_dim = tp.cos_first = 0;
  if (h->gdp) { tp.enc_dim = h->cfg.inner_channel; tp.hid_dim = tp.t_dim = 4 * h->cfg.inner_channel; tp.cos_first = 1; }
  HIPCHK(h, launch_temb(tp, st));
  return FDSR_OK;
}

// Row t of the table is what the per-step kernel would produce for noise level t: same kernel,
// same arithmetic, evaluated for all T levels in one launch.
int build_temb_table(fdsr_handle h, hipStream_t st) {
  if (h->d_temb_table) { (void)hipFree(h->d_temb_table); h->d_temb_table = nullptr; }
  if (h->d_nl) { (void)hipFree(h->d_nl); h->d_nl = nullptr; }
  HIPCHK(h, hipMalloc(&h->d_temb_table, (size_t)h->T * h->TE * sizeof(float)));
  HIPCHK(h, hipMalloc(&h->d_nl, (size_t)h->T * sizeof(float)));
  std::vector<float> nl(h->T);
  for (int t = 0; t < h->T; ++t) nl[t] = (h->sr3 || h->gdp) ? (float)t : h->s_nl[t];
  HIPCHK(h, hipMemcpy(h->d_nl, nl.data(), nl.size() * sizeof(float), hipMemcpyHostToDevice));
  int rc = fill_temb(h, h->d_temb_table, h->T, h->d_nl, 0.f, st);
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(st));
  return FDSR_OK;
}

int ensure_rng(fdsr_handle h) {
  if (h->d_rng) return FDSR_OK;
  HIPCHK(h, hipMalloc(&h->d_rng, 2 * sizeof(unsigned long long)));
  const unsigned long long init[2] = {h->rng_seed, 0ull};
  HIPCHK(h, hipMemcpy(h->d_rng, init, sizeof(init), hipMemcpyHostToDevice));
  return FDSR_OK;
}

StepRecord* step_rec(fdsr_handle h) { return reinterpret_cast<StepRecord*>(reinterpret_cast<char*>(h->d_step_ctl) + 256); }

int upload_step_sched(fdsr_handle h) {
  if (!h->d_step_ctl) {
    HIPCHK(h, hipMalloc(&h->d_step_ctl, 256 + sizeof(StepRecord)));
    HIPCHK(h, hipMemset(h->d_step_ctl, 0, 256 + sizeof(StepRecord)));
    HIPCHK(h, hipMalloc(&h->d_step_row, (size_t)h->TE * sizeof(float)));
  }
  if (h->d_step_sched) { (void)hipFree(h->d_step_sched); h->d_step_sched = nullptr; }
  HIPCHK(h, hipMalloc(&h->d_step_sched, (size_t)5 * h->T * sizeof(float)));
  std::vector<float> s;
  s.reserve((size_t)5 * h->T);
  for (const auto* v : {&h->s_recip, &h->s_recipm1, &h->s_c1, &h->s_c2, &h->s_sigma}) s.insert(s.end(), v->begin(), v->end());
  HIPCHK(h, hipMemcpy(h->d_step_sched, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice));
  return FDSR_OK;
}

// ---- the loop ---------------------------------------------------------------------------------------------------------------
// one sampling call: the caller's arguments, and what sample_prepare made of them
struct SampleCall {
  const float *cond, *noise;
  float *out, *traj;
  int N, H, W;
  int every;          // fdsr_sample_stepwise: the trajectory keeps the steps with t % every == 0
  NoiseTiles tiles;   // the handle's noise-tile table where the call draws its own noise (sample_prepare); else none
  char* ws;
  hipStream_t st;
  bool use_graph;
};

// everything before step 0: the range flag, the packed input, the call counter of the engine's noise, and (where the steps
// read it) k = 0
int sample_head(fdsr_handle h, const SampleCall& c, bool reset_counter) {
  float* xin = reinterpret_cast<float*>(c.ws + h->plan.tensor_off[h->t_in]);
  // x_in = cond, img = randn(shape)                                       diffusion.py:204-208
  // packed input: cat([cond, x_t]) (diffusion.py:173); GDP: cat([x_t, cond]) (gdp_modules/diffusion.py:191)
  const int x_off = h->gdp ? 0 : 3, c_off = h->gdp ? 3 : 0;
  // the f16x3 range flag speaks for THIS call only (a captured loop clears it at every replay)
  if (h->prec == PREC_F16X3 && g_tun.sat_guard) HIPCHK(h, hipMemsetAsync(h->d_sat, 0, sizeof(int), c.st));
  HIPCHK(h, launch_nchw_to_nhwc(c.cond, xin, c.N, 3, c.H, c.W, h->CP, c_off, 1, c.st));
  if (c.noise) {
    HIPCHK(h, launch_nchw_to_nhwc(c.noise, xin, c.N, 3, c.H, c.W, h->CP, x_off, 0, c.st));
  } else {   // the engine draws: a new call counter per sample (also under graph replay), plane 0 = x_T
    // tile-addressed noise: the counter stays where it is, so every group of a scene draws from the one field of that counter
    if (!c.tiles.origins) HIPCHK(h, launch_rng_advance(h->d_rng, c.st));
    HIPCHK(h, launch_randn_xin(h->d_rng, xin, c.N, c.H * c.W, h->CP, c.st, x_off, c.tiles));
  }
  if (reset_counter) HIPCHK(h, hipMemsetAsync(h->d_step_ctl, 0, sizeof(int), c.st));
  return FDSR_OK;
}

// One reverse step: the UNet with a noise-embedding row, then the posterior update.  k >= 0: the host knows the step, the row is
// its row of the table and the scalars are kernel arguments.  DEVICE_STEP: the step is whichever the device counter holds --
// the prologue copies its row and fills its record -- so the launches are identical for every k.
constexpr int DEVICE_STEP = -1;

int sample_step(fdsr_handle h, const SampleCall& c, int k) {
  const int t = k == DEVICE_STEP ? -1 : h->T - 1 - k;                       // for i in reversed(range(T))  :209 (-1: only the device knows it)
  const float* row = h->d_step_row;
  const int base_prec = h->prec;
  if (k == DEVICE_STEP) {
    StepPrologueParams sp{};
    sp.counter = h->d_step_ctl;
    sp.sched = h->d_step_sched;
    sp.temb_table = h->d_temb_table;
    sp.temb_row = h->d_step_row;
    sp.rec = step_rec(h);
    sp.T = h->T; sp.TE = h->TE; sp.traj_every = c.every;
    HIPCHK(h, launch_step_prologue(sp, c.st));
  } else {
    // FastDiffSR: the network sees the noise level sqrt(alpha_bar) (:169-170); SR3: the integer time
    row = h->d_temb_table + (size_t)t * h->TE;
    // (probe "bf16_f16x3_steps": this step on the fp32-grade kernels; the plan, the workspace and both 16-bit weight forms serve either mode,
    // x_t and the network output cross a step as fp32)
    const int fs = g_tun.bf16_f16x3_steps;
    if (base_prec == PREC_BF16 && ((fs > 0 && k < fs) || (fs < 0 && k >= h->T + fs))) h->prec = PREC_F16X3;
  }
  int rc = run_unet(h, c.N, c.H, c.W, c.ws, nullptr, 0.f, c.st, row);
  h->prec = base_prec;
  if (rc) return rc;
  // what both posterior kernels take alike; a device step passes the bases, and its record picks the noise plane, the
  // trajectory slot and whether out is written
  auto fill = [&](auto& pp, const float* noise, float* traj, float* out) {
    pp.eps = reinterpret_cast<const float*>(c.ws + h->plan.tensor_off[h->t_eps]);
    pp.xin = reinterpret_cast<float*>(c.ws + h->plan.tensor_off[h->t_in]);
    pp.noise = noise;
    pp.rng = c.noise ? nullptr : h->d_rng;
    pp.tiles = c.tiles;
    pp.traj = traj;
    pp.out = out;
    pp.N = c.N; pp.HW = c.H * c.W; pp.CP = h->CP;
    pp.x_off = h->gdp ? 0 : 3; pp.x0_pred = h->gdp ? 1 : 0;
    pp.plain_out = h->plain_out ? 1 : 0;                                        // ddpm_modules: ret_img[-1] is x_0 itself
  };
  if (k == DEVICE_STEP) {
    PosteriorStepParams pp{};
    fill(pp, c.noise, c.traj, c.out);
    pp.rec = step_rec(h);
    HIPCHK(h, launch_posterior_step(pp, c.st));
    return FDSR_OK;
  }
  const size_t img = (size_t)c.N * 3 * c.H * c.W;
  PosteriorParams pp{};
  fill(pp, (t > 0 && c.noise) ? c.noise + (size_t)(k + 1) * img : nullptr,   // zeros at t == 0  :189
       c.traj ? c.traj + (size_t)k * img : nullptr, t == 0 ? c.out : nullptr);
  if (t == 0) pp.rng = nullptr;
  pp.rng_plane = k + 1;
  pp.c_recip = h->s_recip[t]; pp.c_recipm1 = h->s_recipm1[t];
  pp.coef1 = h->s_c1[t]; pp.coef2 = h->s_c2[t]; pp.sigma = h->s_sigma[t];
  HIPCHK(h, launch_posterior(pp, c.st));
  return FDSR_OK;
}

// head and T steps, eagerly (under profiling only every 4th step's convs are bracketed by events); the capture of fdsr_sample's
// whole loop runs it too
int sample_loop(fdsr_handle h, const SampleCall& c, bool device_steps) {
  int rc = sample_head(h, c, device_steps);
  for (int k = 0; k < h->T && !rc; ++k) {
    h->prof_step = (k % 4) == 0;
    rc = sample_step(h, c, device_steps ? DEVICE_STEP : k);
  }
  h->prof_step = true;
  return rc;
}

// ---- captured graphs --------------------------------------------------------------------------------------------------------
int capture_exec(fdsr_handle h, hipStream_t st, const std::function<int()>& body, hipGraphExec_t* exec) {
  hipGraph_t graph = nullptr;
  HIPCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = body();
  hipError_t e = hipStreamEndCapture(st, &graph);
  if (rc || e != hipSuccess) {   // a failing body wins over a failing end of capture
    if (graph) (void)hipGraphDestroy(graph);
    return rc ? rc : fail(h, FDSR_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  }
  e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) return fail(h, FDSR_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  return FDSR_OK;
}

void destroy_graph(const SampleGraph& g) {
  for (hipGraphExec_t x : g.exec)
    if (x) (void)hipGraphExecDestroy(x);
}

void drop_captures(fdsr_handle h) {
  for (auto* list : {&h->graphs, &h->step_graphs}) {
    for (auto& g : *list) destroy_graph(g);
    list->clear();
  }
}

// The call, eagerly or as graphs.  chunk == 0 (fdsr_sample): the whole loop is one graph, all per-step scalars are kernel
// arguments.  Else (fdsr_sample_stepwise) the steps read the device counter: the head, `chunk` steps and the T % chunk
// remainder are three single-stream captures, and the chunk replays T / chunk times.
int run_sample(fdsr_handle h, const SampleCall& c, int chunk) {
  const bool device_steps = chunk > 0;
  if (!c.use_graph) return sample_loop(h, c, device_steps);
  if (h->graphs_epoch != g_tun.epoch) {   // graphs captured under other launcher options
    drop_captures(h);
    h->graphs_epoch = g_tun.epoch;
  }
  std::vector<SampleGraph>& list = device_steps ? h->step_graphs : h->graphs;
  const SampleGraph* g = nullptr;
  for (const auto& e : list)
    if (e.cond == c.cond && e.noise == c.noise && e.out == c.out && e.traj == c.traj && e.ws == c.ws &&
        e.temb_table == h->d_temb_table && e.sched == h->d_step_sched && e.N == c.N && e.H == c.H && e.W == c.W &&
        e.chunk == chunk && e.every == c.every && e.tiles == c.tiles.origins && e.scene_w == c.tiles.scene_w)
      g = &e;
  const int T = h->T;
  if (!g) {
    SampleGraph ge{c.cond, c.noise, c.out, c.traj, c.ws, h->d_temb_table, h->d_step_sched, c.N, c.H, c.W, chunk, c.every,
                   c.tiles.origins, c.tiles.scene_w, {}};
    auto steps = [&](int n) {
      int r = FDSR_OK;
      for (int k = 0; k < n && !r; ++k) r = sample_step(h, c, DEVICE_STEP);
      return r;
    };
    int rc;
    if (!device_steps) {
      rc = capture_exec(h, c.st, [&] { return sample_loop(h, c, false); }, &ge.exec[0]);
    } else {
      rc = capture_exec(h, c.st, [&] { return sample_head(h, c, true); }, &ge.exec[0]);
      if (!rc) rc = capture_exec(h, c.st, [&] { return steps(chunk); }, &ge.exec[1]);
      if (!rc && T % chunk) rc = capture_exec(h, c.st, [&] { return steps(T % chunk); }, &ge.exec[2]);
    }
    if (rc) { destroy_graph(ge); return rc; }
    if (list.size() >= 8) {   // at most 8 per entry point (include/fdsr.h): the oldest goes
      destroy_graph(list.front());
      list.erase(list.begin());
    }
    list.push_back(ge);
    g = &list.back();
  }
  HIPCHK(h, hipGraphLaunch(g->exec[0], c.st));
  for (int i = 0; device_steps && i < T / chunk; ++i) HIPCHK(h, hipGraphLaunch(g->exec[1], c.st));
  if (g->exec[2]) HIPCHK(h, hipGraphLaunch(g->exec[2], c.st));
  return FDSR_OK;
}

// What both entry points check before they run, in this order; `refusal`: fdsr_sample_stepwise's own, reported where it always was.
// Sets c->ws, the stream and whether the call runs captured (profiling brackets launches with events: eager).
int sample_prepare(fdsr_handle h, SampleCall* c, void* workspace, size_t workspace_bytes, void* hip_stream, int flags, bool stepwise,
                   const char* refusal) {
  if (!h || !c->cond || !c->out) return fail(h, FDSR_E_INVALID, "null argument");
  if (h->cfg.in_channel != 6 || h->cfg.out_channel != 3)
    return fail(h, FDSR_E_INVALID, "conditional sampling needs in_channel=6, out_channel=3");
  if (refusal) return fail(h, FDSR_E_INVALID, "%s", refusal);
  int rc = plan_ready(h, true, c->N, c->H, c->W, workspace, workspace_bytes);
  if (rc) return rc;
  c->st = reinterpret_cast<hipStream_t>(hip_stream);
  c->ws = reinterpret_cast<char*>(workspace);
  if ((rc = apply_plan(h, fdsr_forms::need_sample(h->forms, h->prec, stepwise), c->st))) return rc;   // optimiser steps moved the master copy
  if (!c->noise && (rc = ensure_rng(h))) return rc;
  if (!c->noise && !h->noise_tiles.for_call(c->N, c->W, &c->tiles))   // the table counts where the call draws its own noise
    return fail(h, FDSR_E_INVALID, "a call of %d images under a noise-tile table of %d (fdsr_set_noise_tiles)", c->N, h->noise_tiles.n);
  if ((flags & FDSR_SAMPLE_GRAPH) && c->st == nullptr)
    return fail(h, FDSR_E_INVALID, "FDSR_SAMPLE_GRAPH needs a non-default stream (stream capture cannot run on the NULL stream)");
  c->use_graph = (flags & FDSR_SAMPLE_GRAPH) && !h->profiling;
  return FDSR_OK;
}

// default chunk: T itself up to 32 steps, else the largest divisor of T in [16, 32] (T = 1000 / 2000: 25), else 32 + a remainder
int default_chunk(int T) {
  if (T <= 32) return T;
  for (int c = 32; c >= 16; --c)
    if (T % c == 0) return c;
  return 32;
}

}  // namespace fdsr_int

extern "C" {

int fdsr_sample(fdsr_handle h, const float* cond_nchw, const float* noise, float* out_nchw, float* traj_nchw, int batch,
                int height, int width, void* workspace, size_t workspace_bytes, void* hip_stream, int flags) {
  SampleCall c{cond_nchw, noise, out_nchw, traj_nchw, batch, height, width, 1, {}};
  const int rc = sample_prepare(h, &c, workspace, workspace_bytes, hip_stream, flags, false, nullptr);
  return rc ? rc : run_sample(h, c, 0);
}

int fdsr_sample_stepwise(fdsr_handle h, const float* cond_nchw, const float* noise, float* out_nchw, float* traj_nchw, int batch,
                         int height, int width, void* workspace, size_t workspace_bytes, void* hip_stream, int flags,
                         const fdsr_sample_opts* opts) {
  const int chunk_opt = opts ? opts->chunk_steps : 0, every = opts ? opts->traj_every : 1;
  const char* refusal = nullptr;
  if (chunk_opt < 0 || every < 1) refusal = "fdsr_sample_opts: chunk_steps >= 0 and traj_every >= 1";
  else if (g_tun.bf16_f16x3_steps != 0)
    refusal = "fdsr_sample_stepwise: the bf16_f16x3_steps probe makes the precision step-dependent; use fdsr_sample";
  SampleCall c{cond_nchw, noise, out_nchw, traj_nchw, batch, height, width, every, {}};
  const int rc = sample_prepare(h, &c, workspace, workspace_bytes, hip_stream, flags, true, refusal);
  if (rc) return rc;
  if (c.use_graph && h->training && h->n_drop_slots > 0)   // a replayed chunk would repeat its dropout masks
    return fail(h, FDSR_E_INVALID, "fdsr_sample_stepwise: FDSR_SAMPLE_GRAPH with live dropout (train mode); sample eagerly");
  return run_sample(h, c, chunk_opt > 0 ? std::min(chunk_opt, h->T) : default_chunk(h->T));
}

int fdsr_set_seed(fdsr_handle h, uint64_t seed) {
  if (!h) return FDSR_E_INVALID;
  h->rng_seed = seed;
  h->drop_seed = seed;   // one seed call covers both generators unless fdsr_set_dropout_seed overrides it
  h->drop_step = 0;
  if (h->d_rng) {
    const unsigned long long init[2] = {seed, 0ull};
    HIPCHK(h, hipMemcpy(h->d_rng, init, sizeof(init), hipMemcpyHostToDevice));
  }
  return FDSR_OK;
}

int fdsr_randn(fdsr_handle h, float* dst_nchw, int batch, int height, int width, int plane, void* hip_stream) {
  if (!h || !dst_nchw || batch < 1 || height < 1 || width < 1 || plane < 0) return fail(h, FDSR_E_INVALID, "bad fdsr_randn arguments");
  int rc = ensure_rng(h);
  if (rc) return rc;
  NoiseTiles tiles;
  if (!h->noise_tiles.for_call(batch, width, &tiles))
    return fail(h, FDSR_E_INVALID, "fdsr_randn: %d images under a noise-tile table of %d (fdsr_set_noise_tiles)", batch, h->noise_tiles.n);
  HIPCHK(h, launch_randn_plane(h->d_rng, dst_nchw, batch, height * width, plane, reinterpret_cast<hipStream_t>(hip_stream), 0, tiles));
  return FDSR_OK;
}

int fdsr_set_noise_tiles(fdsr_handle h, const int32_t* origins_dev, int n_tiles, int scene_w) {
  if (!h) return FDSR_E_INVALID;
  if (!h->noise_tiles.set(origins_dev, n_tiles, scene_w))
    return fail(h, FDSR_E_INVALID, "fdsr_set_noise_tiles: a table needs n_tiles >= 1 and scene_w >= 1 (got %d, %d)", n_tiles, scene_w);
  return FDSR_OK;
}

}  // extern "C"
