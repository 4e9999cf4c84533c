// The host scaffold of the transformer families (fdsr_swinir.hip, fdsr_hat.hip, fdsr_transenet.hip): the bookkeeping of the
// TABLE / SIZE / RUN walk, the engine object, and the frames of create, destroy, load, workspace_bytes, forward and debug_tensor.
// A family writes its network as `struct Walker : WalkerBase<F>` with a walk(), and describes itself in a traits struct F:
//   Config, Desc, Walk, Obj   its fdsr_*_config, its LayerDesc (name, kind, cin, cout; tensors(), tensor_name(j), shape(j)),
//                             its Walker and its fdsr_*_obj (struct fdsr_*_obj : Engine<F> {})
//   name, graph_flag_name     "fdsr_hat" and "FDSR_HAT_GRAPH", for messages
//   NBUF, SIDE, graph_flag    the workspace buffers, a legal image side for the TABLE walk, FDSR_*_GRAPH
//   check_shape(fn, B, H, W)  which images it computes
//   pack(L, j, host, packed)  tensor j of layer L as the device holds it
//   canonical_name(cfg, name) the table's name of a checkpoint key; after_load(s, layer): what else a loaded tensor needs
//                             (FamilyDefaults: the key itself, nothing)
// Nothing here asks which family it serves.  The extern "C" functions check their own configuration, then call a frame with
// their name for the messages.
#pragma once
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "fdsr_swin_common.h"

namespace {

struct Graph { int B, H, W; const void *x, *out, *ws; hipGraphExec_t exec; };

template <class F>
struct Engine {
  typename F::Config cfg{};
  std::vector<typename F::Desc> table;
  std::vector<std::string> taps;
  std::vector<unsigned char> have;   // [layer * 2 + j]
  std::vector<float*> w, b;          // device: tensor 0 and tensor 1 of each layer, as F::pack lays them out
  std::vector<Graph> graphs;
};

struct FamilyDefaults {
  template <class C> static std::string canonical_name(const C&, const char* name) { return name; }
  template <class E> static int after_load(E&, int) { return FDSR_OK; }
};

// The network is written once, as a walk: the same code lists the checkpoint tensors in load order (TABLE), sizes the workspace
// (SIZE) and launches the kernels (RUN).
template <class F>
struct WalkerBase {
  using Kind = decltype(F::Desc::kind);
  Mode mode = RUN;
  typename F::Config cfg{};
  std::vector<typename F::Desc>* table = nullptr;   // TABLE: appended to
  std::vector<std::string>* taps = nullptr;         // TABLE: the tap names, appended to
  size_t need[F::NBUF] = {};                        // SIZE: floats per image of each buffer
  int N = 0, Hin = 0, Win = 0;
  const float* img = nullptr;                       // RUN: the input, NCHW
  float* dst = nullptr;                             // RUN: the output, NCHW (null: a debug walk, which ends at `stop`)
  float* buf[F::NBUF] = {};
  float* const* w = nullptr;
  float* const* b = nullptr;
  hipStream_t st = nullptr;
  int li = 0;                                       // the next layer's index (load order)
  int reuse = -1;                                   // >= 0: the next layer() is this layer again (a module the network runs twice)
  const char* stop = nullptr;                       // RUN: the tap to end at
  bool done = false;
  T tapped{};
  int err = FDSR_OK;

  bool live() const { return mode == RUN && err == FDSR_OK && !done; }
  bool stops_at(const std::string& name) const { return live() && stop && name == stop; }
  void touch(const T& t) { need[t.buf] = std::max(need[t.buf], (size_t)t.H * t.W * t.C); }
  void check(hipError_t e) {
    if (e != hipSuccess && err == FDSR_OK) err = fail(nullptr, FDSR_E_HIP, "%s: kernel launch failed: %s", F::name, hipGetErrorString(e));
  }
  void tap(const std::string& name, const T& t) {
    if (mode == TABLE) taps->push_back(name);
    if (stops_at(name)) { done = true; tapped = t; }
  }
  int layer(const std::string& name, Kind kind, int cin, int cout) {
    if (reuse >= 0) {
      const int idx = reuse;
      reuse = -1;
      return idx;
    }
    if (mode == TABLE) table->push_back(typename F::Desc{name, kind, cin, cout});
    return li++;
  }

  // the GemmArgs fields of layer idx that do not depend on the gather or the epilogue: `in` as rows of pixels, K = cin or 9 cin
  void gemm_args(GemmArgs& a, int idx, const T& in, const T* res, bool conv, int cin, int cout, int r) const {
    a.x = buf[in.buf];
    a.w = w[idx];
    a.bias = b[idx];
    a.res = res ? buf[res->buf] : nullptr;
    a.M = N * in.H * in.W;
    a.N = cout;
    a.K = conv ? 9 * cin : cin;
    a.Kpad = gemm_kpad(conv, cin);
    a.Npad = gemm_npad(cout);
    a.H = in.H;
    a.W = in.W;
    a.Cin = in.C;
    a.r = r;
  }

  // LayerNorm of layer idx (gamma in w, beta in b)
  T norm(int idx, const T& in, int ob) {
    T out{ob, in.H, in.W, in.C};
    if (mode == SIZE) touch(out);
    if (!live()) return out;
    const int M = N * in.H * in.W;
    hipLaunchKernelGGL(swin_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, buf[in.buf], w[idx], b[idx], buf[ob], M, in.C);
    check(hipGetLastError());
    return out;
  }
};

template <class F>
typename F::Walk walker(const Engine<F>* s, Mode mode, int B, int H, int W) {
  typename F::Walk wk;
  wk.mode = mode;
  wk.cfg = s->cfg;
  wk.N = B;
  wk.Hin = H;
  wk.Win = W;
  return wk;
}

template <int NBUF>
struct Plan { size_t off[NBUF]; size_t bytes; };

template <class F>
Plan<F::NBUF> make_plan(const Engine<F>* s, int B, int H, int W) {
  typename F::Walk wk = walker(s, SIZE, B, H, W);
  wk.walk();
  Plan<F::NBUF> pl{};
  size_t off = 0;
  for (int i = 0; i < F::NBUF; ++i) {
    pl.off[i] = off;
    off = align_up(off + (size_t)B * wk.need[i] * sizeof(float), 256);
  }
  pl.bytes = off;
  return pl;
}

template <class F>
void drop_graphs(Engine<F>* s) {
  for (Graph& g : s->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  s->graphs.clear();
}

// everything a forward or a debug walk checks, then the walker ready to run
template <class F>
int prepare(Engine<F>* s, const char* fn, const float* x, int B, int H, int W, void* ws, size_t ws_bytes, void* stream, typename F::Walk* out) {
  if (!s || !x || !ws) return fail(nullptr, FDSR_E_INVALID, "%s: null argument", fn);
  int rc = F::check_shape(fn, B, H, W);
  if (rc) return rc;
  for (size_t L = 0; L < s->table.size(); ++L)
    for (int j = 0; j < s->table[L].tensors(); ++j)
      if (!s->have[L * 2 + j]) return fail(nullptr, FDSR_E_STATE, "%s: tensor '%s' is missing", fn, s->table[L].tensor_name(j).c_str());
  const Plan<F::NBUF> pl = make_plan(s, B, H, W);
  if (ws_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(ws) & 255))
    return fail(nullptr, FDSR_E_WORKSPACE, "%s: workspace too small (%zu < %zu bytes) or not 256-byte aligned", fn, ws_bytes, pl.bytes);
  typename F::Walk wk = walker(s, RUN, B, H, W);
  wk.img = x;
  for (int i = 0; i < F::NBUF; ++i) wk.buf[i] = reinterpret_cast<float*>(static_cast<char*>(ws) + pl.off[i]);
  wk.w = s->w.data();
  wk.b = s->b.data();
  wk.st = reinterpret_cast<hipStream_t>(stream);
  *out = wk;
  return FDSR_OK;
}

// the end of fdsr_*_create, after the family's checks of cfg
template <class F>
int engine_create(const char* fn, const typename F::Config& cfg, typename F::Obj** out) {
  typename F::Obj* s = new (std::nothrow) typename F::Obj();
  if (!s) return fail(nullptr, FDSR_E_INVALID, "%s: out of host memory", fn);
  s->cfg = cfg;
  typename F::Walk wk = walker<F>(s, TABLE, 1, F::SIDE, F::SIDE);
  wk.table = &s->table;
  wk.taps = &s->taps;
  wk.walk();
  s->have.assign(s->table.size() * 2, 0);
  s->w.assign(s->table.size(), nullptr);
  s->b.assign(s->table.size(), nullptr);
  *out = s;
  return FDSR_OK;
}

template <class F>
void engine_destroy(typename F::Obj* s) {
  if (!s) return;
  drop_graphs<F>(s);
  for (float* p : s->w)
    if (p) (void)hipFree(p);
  for (float* p : s->b)
    if (p) (void)hipFree(p);
  delete s;
}

template <class F>
int engine_load(const char* fn, Engine<F>* s, const char* name, const float* host_f32, const int64_t* shape, int ndim) {
  if (!s || !name || !host_f32 || (ndim > 0 && !shape) || ndim < 0) return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments", fn);
  const std::string nm = F::canonical_name(s->cfg, name);
  int layer = -1, j = -1;
  for (size_t L = 0; L < s->table.size() && layer < 0; ++L)
    for (int q = 0; q < s->table[L].tensors(); ++q)
      if (s->table[L].tensor_name(q) == nm) { layer = (int)L; j = q; break; }
  if (layer < 0) return fail(nullptr, FDSR_E_KEY, "%s: unknown tensor '%s'", fn, name);
  const typename F::Desc& L = s->table[layer];
  const std::vector<int64_t> want = L.shape(j);
  if (ndim != (int)want.size() || !std::equal(want.begin(), want.end(), shape))
    return fail(nullptr, FDSR_E_KEY, "%s: '%s' has the wrong shape", fn, name);
  std::vector<float> packed;
  F::pack(L, j, host_f32, packed);
  float*& dst = j == 0 ? s->w[layer] : s->b[layer];
  // a running forward may still read the old values, and a captured graph holds them: loading is host-synchronous and drops
  // the graphs
  HIPCHK(nullptr, hipDeviceSynchronize());
  drop_graphs(s);
  if (!dst) HIPCHK(nullptr, hipMalloc(reinterpret_cast<void**>(&dst), packed.size() * sizeof(float)));
  HIPCHK(nullptr, hipMemcpy(dst, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
  const int rc = F::after_load(*s, layer);
  if (rc) return rc;
  s->have[(size_t)layer * 2 + j] = 1;
  return FDSR_OK;
}

template <class F>
int engine_workspace_bytes(const char* fn, Engine<F>* s, int B, int H, int W, size_t* bytes) {
  if (!s || !bytes) return fail(nullptr, FDSR_E_INVALID, "%s: null argument", fn);
  const int rc = F::check_shape(fn, B, H, W);
  if (rc) return rc;
  *bytes = make_plan(s, B, H, W).bytes;
  return FDSR_OK;
}

template <class F>
int engine_forward(const char* fn, Engine<F>* s, const float* x, int B, int H, int W, float* out, void* ws, size_t ws_bytes, void* stream,
                   int flags) {
  if (!out || (flags & ~F::graph_flag)) return fail(nullptr, FDSR_E_INVALID, "%s: bad arguments", fn);
  if ((flags & F::graph_flag) && !stream) return fail(nullptr, FDSR_E_INVALID, "%s: %s needs a created stream", fn, F::graph_flag_name);
  typename F::Walk wk;
  int rc = prepare(s, fn, x, B, H, W, ws, ws_bytes, stream, &wk);
  if (rc) return rc;
  wk.dst = out;
  if (!(flags & F::graph_flag)) {
    wk.walk();
    return wk.err;
  }
  // one graph per (B, H, W); other pointers under the same shape capture anew
  Graph* g = nullptr;
  for (Graph& q : s->graphs)
    if (q.B == B && q.H == H && q.W == W) g = &q;
  if (g && !(g->x == x && g->out == out && g->ws == ws)) {
    (void)hipGraphExecDestroy(g->exec);
    s->graphs.erase(s->graphs.begin() + (g - s->graphs.data()));
    g = nullptr;
  }
  if (!g) {
    hipGraphExec_t exec = nullptr;
    if ((rc = capture_exec(nullptr, wk.st, [&]() -> int { wk.walk(); return wk.err; }, &exec))) return rc;
    s->graphs.push_back(Graph{B, H, W, x, out, ws, exec});
    g = &s->graphs.back();
  }
  HIPCHK(nullptr, hipGraphLaunch(g->exec, wk.st));
  return FDSR_OK;
}

template <class F>
int engine_debug_tensor(const char* fn, Engine<F>* s, const char* name, const float* x, int B, int H, int W, float* out_nhwc,
                        size_t capacity_floats, int* dims3, void* ws, size_t ws_bytes, void* stream) {
  if (!name || !out_nhwc || !dims3) return fail(nullptr, FDSR_E_INVALID, "%s: null argument", fn);
  typename F::Walk wk;
  const int rc = prepare(s, fn, x, B, H, W, ws, ws_bytes, stream, &wk);
  if (rc) return rc;
  // the name is checked before anything runs: a walk that meets no tap would go on to the network's last store, and a debug walk
  // has no output
  const bool known = std::find(s->taps.begin(), s->taps.end(), std::string(name)) != s->taps.end();
  if (!known) return fail(nullptr, FDSR_E_KEY, "%s: unknown tap '%s'", fn, name);
  wk.stop = name;
  wk.walk();
  if (wk.err) return wk.err;
  if (!wk.done) return fail(nullptr, FDSR_E_KEY, "%s: tap '%s' was not reached", fn, name);
  const T& tp = wk.tapped;
  const size_t count = (size_t)B * tp.H * tp.W * tp.C;
  if (count > capacity_floats) return fail(nullptr, FDSR_E_INVALID, "%s: '%s' needs %zu floats", fn, name, count);
  dims3[0] = tp.H; dims3[1] = tp.W; dims3[2] = tp.C;
  HIPCHK(nullptr, hipMemcpyAsync(out_nhwc, wk.buf[tp.buf], count * sizeof(float), hipMemcpyDeviceToDevice, wk.st));
  return FDSR_OK;
}

}  // namespace
