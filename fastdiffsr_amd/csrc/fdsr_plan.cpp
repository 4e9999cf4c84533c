// The static plan of libfdsr_hip.so: op list, tensors and checkpoint schema of the UNets, derived from the same hyper-parameters the
// reference's factory passes to unet.UNet (model/networks.py:94-104).  Two builders -- the flagship with its SR3 / TESR siblings
// (UNet.__init__/forward, model/fastdiffsr_modules/unet.py:224-323) and the GDP sibling -- put their plans together from the helpers
// of one PlanBuilder.  Pure host code; fdsr_create calls build_plan, everything shape-dependent is fdsr_engine.cpp's.
//
// The order of the calls IS the plan: add_weight follows state_dict() (per module, registration order), new_tensor numbers the
// workspace tensors, a GroupNorm op sits directly in front of its convolution, GroupNorm and dropout slots count in network order.
// Every helper below allocates top to bottom as written; callers allocate into named locals, never inside an argument list.
#include <algorithm>
#include <string>
#include <vector>

#include "fdsr_engine_int.h"

using namespace fdsr;
using namespace fdsr_int;

namespace {

int add_weight(fdsr_handle h, const std::string& key, std::vector<int64_t> shape, bool live) {
  WeightEntry w;
  w.key = key;
  w.shape = std::move(shape);
  w.live = live;
  h->weights.push_back(w);
  h->key2w[key] = (int)h->weights.size() - 1;
  return (int)h->weights.size() - 1;
}

int new_tensor(fdsr_handle h, int C, int level, const std::string& name = "") {
  TensorDesc t;
  t.C = C;
  t.level = level;
  t.name = name;
  h->tensors.push_back(t);
  return (int)h->tensors.size() - 1;
}

// conv weight entry -> packed [tap][Cout_pad][Cin_pad]
void mark_conv_pack(fdsr_handle h, int widx, ConvKind ck, int cin_store, int C0, int C1, int cout) {
  int KC, BN;
  conv_tile_config(ck, C0, C1, cout, &KC, &BN);
  WeightEntry& w = h->weights[widx];
  w.sink = WeightEntry::CONV_PACK;
  w.ks = ck == CONV1 ? 1 : 3;
  w.cin_pad = round_up(cin_store, KC);
  w.cout_pad = round_up(cout, BN);
  w.ck = ck;
  // 16-bit MFMA kernels: 16-channel K chunks; a concat seam must fall on a chunk boundary
  w.h_ok = (cin_store % 16 == 0) && (C1 == 0 || C0 % 16 == 0);
  if (w.h_ok) {
    int TH, WN;
    conv_h_config(ck, cout, &TH, &WN);
    w.h_WN = WN;
    w.h_cin_pad = round_up(cin_store, 16);
    w.h_cout_pad = round_up(cout, 32 * WN);
  }
}

// Shared tail of the plan builders: device layout of the parameters (the per-block embedding Linears concatenated
// into one [TE][row_len] table), master-copy offsets, synthetic entries, 16-bit weight arena, tensor liveness.
int finish_plan(fdsr_handle h, const std::string mlp_keys[4], int row_len) {
  const int ic = row_len;
  // parameter arena layout
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += align_up(n, 64); return o; };
  const size_t noise_w_off = h->noise_w_off = take((size_t)h->TE * ic);
  const size_t noise_b_off = h->noise_b_off = take((size_t)h->TE);
  for (int i = 0; i < 4; ++i) h->w_mlp[i] = h->key2w[mlp_keys[i]];
  for (auto& w : h->weights) {
    if (!w.live) continue;
    switch (w.sink) {
      case WeightEntry::RAW: w.dev_off = take(numel(w.shape)); break;
      case WeightEntry::CONV_PACK: w.dev_off = take((size_t)w.ks * w.ks * w.cout_pad * w.cin_pad); break;
      case WeightEntry::NOISE_W: w.dev_off = noise_w_off + (size_t)w.row_off * ic; break;
      case WeightEntry::NOISE_B: w.dev_off = noise_b_off + (size_t)w.row_off; break;
    }
  }
  h->n_schema = (int)h->weights.size();
  {   // master copy (checkpoint layout) of every live tensor: what the optimiser updates, what fdsr_get_weight returns
    size_t mo = 0;
    h->master_off.assign(h->weights.size(), SIZE_MAX);
    for (int i = 0; i < h->n_schema; ++i) {
      if (!h->weights[i].live) continue;
      h->master_off[i] = mo;
      mo += align_up(numel(h->weights[i].shape), 4);
    }
    h->master_floats = mo;
  }
  if (h->max_qkv) {   // zeros standing in for the missing bias of attn.qkv (Conv2d(bias=False))
    WeightEntry z;
    z.key = "__zero_bias";
    z.shape = {h->max_qkv};
    z.live = false;
    z.loaded = true;
    z.dev_off = take(h->max_qkv);
    h->weights.push_back(z);
    h->w_zero_bias = (int)h->weights.size() - 1;
  }
  // positional-encoding frequency table (not a checkpoint tensor): filled at device init
  if (!h->sr3) {
    WeightEntry f;
    f.key = "__posenc_freq";
    f.shape = {h->freq_count};
    f.live = false;
    f.loaded = true;
    f.dev_off = take(h->freq_count);
    h->weights.push_back(f);
    h->w_freq = (int)h->weights.size() - 1;
  }
  h->param_floats = off;
  // 16-bit weight arena: [cot][kc][wn][tap][plane][lane] x 16 B per conv, for f16x3 (2 planes) and bf16 (1)
  {
    size_t qoff = 0;
    for (auto& w : h->weights) {
      if (!w.live || w.sink != WeightEntry::CONV_PACK || !w.h_ok) continue;
      const size_t frag = (size_t)(w.h_cout_pad / 32) * (w.h_cin_pad / 16) * w.ks * w.ks * 64 * 16;
      w.hq_off[PREC_F16X3] = qoff; qoff += align_up(frag * 2, 256);
      w.hq_off[PREC_BF16] = qoff;  qoff += align_up(frag, 256);
      if (w.ck == CONV3_UP) {   // 16 (parity, tap) slots instead of 9 taps
        const size_t f2 = (size_t)(w.h_cout_pad / 32) * (w.h_cin_pad / 16) * 16 * 64 * 16;
        w.up2_off[PREC_F16X3] = qoff; qoff += align_up(f2 * 2, 256);
        w.up2_off[PREC_BF16] = qoff;  qoff += align_up(f2, 256);
      }
    }
    h->wq_bytes = qoff;
  }

  // liveness
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const Op& op = h->ops[i];
    auto use = [&](int t) { if (t >= 0) h->tensors[t].last_use = (int)i; };
    use(op.src0); use(op.src1); use(op.res);
    if (op.rider >= 0) { use(h->ops[op.rider].src0); use(h->ops[op.rider].src1); }   // the fused launch reads the res_conv input itself
    if (op.aux >= 0) {
      if (h->tensors[op.aux].first_def < 0) h->tensors[op.aux].first_def = (int)i;
      h->tensors[op.aux].last_use = (int)i;
    }
    if (op.dst >= 0) {
      if (h->tensors[op.dst].first_def < 0) h->tensors[op.dst].first_def = (int)i;
      h->tensors[op.dst].last_use = std::max(h->tensors[op.dst].last_use, (int)i);
    }
  }
  return FDSR_OK;
}

struct Src { int x0, C0, x1 = -1, C1 = 0; };   // input of an op: a tensor and its width, or the concatenation of two
struct Norm { int gamma = -1, beta = -1; };    // weight entries of a GroupNorm
struct ConvW { int w = -1, b = -1; };          // weight entries of a convolution (w < 0: there is none)
struct Feat { int t, C; };                     // a skip tensor kept for the up path

// What differs between SelfAttention (ddpm_modules/unet.py:99-127; tesr_modules/unet.py:120-149 is the same module) and GDP's
// AttentionBlock (gdp_modules/unet.py:392-439).  Each builder checks its own divisibility rule (32 / 64) before it calls attention().
struct AttnSpec {
  const char *core, *core_out, *proj;   // suffixes: the ATTN op, its output tensor, the output 1x1 (key and op)
  bool conv1d;                          // weights are Conv1d [Cout][Cin][1], not Conv2d [Cout][Cin][1][1]
  bool qkv_bias;                        // false: Conv2d(bias=False), the op takes the shared zero bias (b = -2)
  int head_channels;                    // 0: one head over all channels
};
const AttnSpec SELF_ATTENTION = {".core", ".o", ".out", false, false, 0};
const AttnSpec ATTENTION_BLOCK = {".attention", ".attention", ".proj_out", true, true, 64};

// Second half of a residual block, the same shape in both families (res_tail)
struct ResTail {
  std::string conv2, fill, out;   // op names of the second conv (its GroupNorm: conv2 + ".gn") and of the 1x1 pre-fill; output tensor
  Norm n2;
  ConvW w2, wfill;                // wfill.w < 0: identity residual
  int film_off = -1;              // GDP: FiLM column of the second GroupNorm
  bool rider = false;             // flagship family: link the pre-fill and the second conv (Op::rider / rider_of)
};

struct PlanBuilder {
  fdsr_handle h;
  int lvl = 0;   // level the network is at
  int te = 0;    // rows of the embedding table handed out so far
  std::string mlp_keys[4];

  // `width`: what the message calls cfg.inner_channel
  int check_config(const char* width) {
    const fdsr_config& c = h->cfg;
    if (c.n_mults < 1 || c.n_mults > FDSR_MAX_MULTS) return fail(h, FDSR_E_INVALID, "n_mults out of range");
    if (c.inner_channel % c.norm_groups != 0 || c.inner_channel % 16 != 0)
      return fail(h, FDSR_E_INVALID, "%s must be a multiple of norm_groups and of 16", width);
    if (c.in_channel < 1 || c.in_channel > 8) return fail(h, FDSR_E_INVALID, "in_channel must be in [1,8]");
    if (c.out_channel < 1 || c.out_channel > 32) return fail(h, FDSR_E_INVALID, "out_channel must be in [1,32]");
    h->CP = 8;
    return FDSR_OK;
  }

  int check_block_channels(const std::string& p, Src x, int Cout) {
    const int Cin = x.C0 + x.C1, G = h->cfg.norm_groups;
    if (Cin % G || Cout % G) return fail(h, FDSR_E_INVALID, "%s: channels not divisible by norm_groups", p.c_str());
    if (Cin % 16 || (x.C1 && x.C0 % 16)) return fail(h, FDSR_E_INVALID, "%s: channel counts must be multiples of 16", p.c_str());
    return FDSR_OK;
  }

  bool attn_res_has(int v) const {
    for (int i = 0; i < h->cfg.n_attn_res && i < FDSR_MAX_MULTS; ++i)
      if (h->cfg.attn_res[i] == v) return true;
    return false;
  }

  // the time / noise-level MLP: Linear(in, hidden) at p.l0, Linear(hidden, out) at p.l1
  void embedding_mlp(const std::string& p, int l0, int l1, int in, int hidden, int out) {
    const std::string k0 = p + "." + std::to_string(l0), k1 = p + "." + std::to_string(l1);
    mlp_keys[0] = k0 + ".weight"; mlp_keys[1] = k0 + ".bias"; mlp_keys[2] = k1 + ".weight"; mlp_keys[3] = k1 + ".bias";
    add_weight(h, mlp_keys[0], {hidden, in}, true);
    add_weight(h, mlp_keys[1], {hidden}, true);
    add_weight(h, mlp_keys[2], {out, hidden}, true);
    add_weight(h, mlp_keys[3], {out}, true);
  }

  void input_tensor() {
    h->t_in = new_tensor(h, h->CP, 0, "input");
    h->tensors[h->t_in].persistent = true;
  }

  Norm norm_weights(const std::string& key, int C) {
    Norm n;
    n.gamma = add_weight(h, key + ".weight", {C}, true);
    n.beta = add_weight(h, key + ".bias", {C}, true);
    return n;
  }

  // key.weight (+ key.bias) of a conv over C0 (+ C1) stored channels, marked for packing.  cin_real: channels of the checkpoint
  // tensor where the stored input is padded (the network input).
  ConvW conv_weights(const std::string& key, ConvKind ck, int C0, int C1, int Cout, int cin_real = 0, bool conv1d = false,
                     bool bias = true) {
    const int ks = ck == CONV1 ? 1 : 3, cin = cin_real ? cin_real : C0 + C1;
    ConvW wb;
    wb.w = add_weight(h, key + ".weight", conv1d ? std::vector<int64_t>{Cout, cin, 1} : std::vector<int64_t>{Cout, cin, ks, ks}, true);
    if (bias) wb.b = add_weight(h, key + ".bias", {Cout}, true);
    mark_conv_pack(h, wb.w, ck, C0 + C1, C0, C1, Cout);
    return wb;
  }

  // a block's embedding Linear(row_len -> rows): rows [te, te + rows) of the concatenated table; returns the first
  int embedding_rows(const std::string& key, int rows, int row_len) {
    const int w = add_weight(h, key + ".weight", {rows, row_len}, true);
    const int b = add_weight(h, key + ".bias", {rows}, true);
    h->weights[w].sink = WeightEntry::NOISE_W;
    h->weights[w].row_off = te;
    h->weights[b].sink = WeightEntry::NOISE_B;
    h->weights[b].row_off = te;
    const int first = te;
    te += rows;
    return first;
  }

  // GroupNorm statistics of x at the current level; returns the slot.  The conv that applies them comes next (normed).
  int gn(const std::string& name, Src x, Norm n, int film_off = -1) {
    Op s;
    s.kind = Op::GN_FINALIZE;
    s.name = name;
    s.src0 = x.x0; s.src1 = x.x1; s.C0 = x.C0; s.C1 = x.C1;
    s.lvl_in = lvl;
    s.gn_slot = h->n_gn_slots++;
    s.gamma = n.gamma; s.beta = n.beta;
    s.film_off = film_off;
    h->tensors[x.x0].need_part = true;
    if (x.x1 >= 0) h->tensors[x.x1].need_part = true;
    h->ops.push_back(s);
    return s.gn_slot;
  }

  // Pushes a CONV op into an existing tensor; the reference is good until the next op is pushed: set the extras by name at once.
  Op& conv(const std::string& name, ConvKind ck, Src x, int Cout, int lvl_in, int lvl_out, ConvW wb, int dst) {
    Op op;
    op.kind = Op::CONV;
    op.name = name;
    op.ck = ck;
    op.src0 = x.x0; op.src1 = x.x1; op.C0 = x.C0; op.C1 = x.C1;
    op.Cout = Cout;
    op.lvl_in = lvl_in; op.lvl_out = lvl_out;
    op.w = wb.w; op.b = wb.b;
    op.dst = dst;
    h->ops.push_back(op);
    return h->ops.back();
  }

  // the GroupNorm of `slot` is this conv's prologue; gamma / beta: the GroupNorm backward of the training step reads them off the conv op
  static void normed(Op& k, int slot, Norm n) { k.gn_slot = slot; k.gamma = n.gamma; k.beta = n.beta; }

  // a conv with weights, bias and an output tensor of its own name, nothing else
  int plain_conv(const std::string& wkey, const std::string& name, ConvKind ck, int src, int C, int Cout, int lvl_in, int lvl_out,
                 int cin_real = 0) {
    const ConvW wb = conv_weights(wkey, ck, C, 0, Cout, cin_real);
    const int dst = new_tensor(h, Cout, lvl_out, name);
    conv(name, ck, {src, C}, Cout, lvl_in, lvl_out, wb, dst);
    return dst;
  }

  // x + out(attention(qkv(norm(x)))): GN -> qkv 1x1 -> softmax(QK^T/sqrt(C)) V -> out 1x1 + x.  q: prefix of the keys and names.
  int attention(const AttnSpec& a, const std::string& q, const std::string& out_name, int x, int C) {
    const Norm n = norm_weights(q + ".norm", C);
    ConvW wq = conv_weights(q + ".qkv", CONV1, C, 0, 3 * C, 0, a.conv1d, a.qkv_bias);
    const ConvW wo = conv_weights(q + a.proj, CONV1, C, 0, C, 0, a.conv1d);
    if (!a.qkv_bias) {
      wq.b = -2;   // the shared zero bias
      h->max_qkv = std::max(h->max_qkv, 3 * C);
    }
    const int heads = a.head_channels ? C / a.head_channels : 1;
    const int slot = gn(q + ".norm", {x, C}, n);
    const int qkv = new_tensor(h, 3 * C, lvl, q + ".qkv");
    Op& kq = conv(q + ".qkv", CONV1, {x, C}, 3 * C, lvl, lvl, wq, qkv);
    normed(kq, slot, n);
    kq.gn_plain = true;
    Op at; at.kind = Op::ATTN; at.name = q + a.core; at.src0 = qkv; at.C0 = C; at.lvl_in = lvl; at.heads = heads;
    at.aux = new_tensor(h, -heads, lvl, q + ".scores");   // C < 0: [N][HW][HW] score scratch of |C| heads, sized in the shape plan
    at.dst = new_tensor(h, C, lvl, q + a.core_out);
    h->ops.push_back(at);
    const int out = new_tensor(h, C, lvl, out_name);
    conv(q + a.proj, CONV1, {at.dst, C}, C, lvl, lvl, wo, out).res = x;
    return out;
  }

  // GroupNorm 2 -> `out` tensor -> optional 1x1 of the raw (concatenated) block input x, written into `out` first -> second conv
  // over h1 with the residual (xres, or `out` after the pre-fill) -> its dropout slot
  int res_tail(const ResTail& t, Src x, int xres, int h1, int Cout) {
    const int slot = gn(t.conv2 + ".gn", {h1, Cout}, t.n2, t.film_off);
    const int out = new_tensor(h, Cout, lvl, t.out);
    int fill_idx = -1;
    if (t.wfill.w >= 0) {
      fill_idx = (int)h->ops.size();
      Op& kr = conv(t.fill, CONV1, x, Cout, lvl, lvl, t.wfill, out);
      kr.no_part = true;
      if (t.rider) kr.rider_of = fill_idx + 1;   // the second conv comes next: on the 16-bit kernels it can carry this conv as a rider (run_unet)
      xres = out;
    }
    Op& k2 = conv(t.conv2, CONV3_S1, {h1, Cout}, Cout, lvl, lvl, t.w2, out);
    normed(k2, slot, t.n2);
    k2.res = xres;
    if (t.rider) k2.rider = fill_idx;
    if (h->cfg.dropout > 0.f) k2.drop_slot = h->n_drop_slots++;   // block2 = Block(dim_out, dim_out, dropout=dropout), unet.py:112
    return out;
  }

  // GroupNorm -> Swish -> conv3x3 to out_channel: the network output
  void output_head(const std::string& name, const std::string& norm_key, const std::string& conv_key, int x, int C) {
    const int Cout = h->cfg.out_channel;
    const Norm n = norm_weights(norm_key, C);
    const ConvW wb = conv_weights(conv_key, CONV3_S1, C, 0, Cout);
    const int slot = gn(name + ".gn", {x, C}, n);
    h->t_eps = new_tensor(h, Cout, lvl, name);
    normed(conv(name, CONV3_S1, {x, C}, Cout, lvl, lvl, wb, h->t_eps), slot, n);
    h->tensors[h->t_eps].persistent = true;
  }

  int finish(int row_len, int freq_count) {
    if (lvl != 0) return fail(h, FDSR_E_INVALID, "internal: level bookkeeping");
    h->TE = te;
    h->temb_in = row_len;
    h->freq_count = freq_count;
    return finish_plan(h, mlp_keys, row_len);
  }
};

// The flagship and its SR3 / TESR siblings.  unet.py:224-323.
int build_plan_unet(fdsr_handle h) {
  const fdsr_config& c = h->cfg;
  const int ic = c.inner_channel, G = c.norm_groups;
  PlanBuilder b{h};
  h->sr3 = c.variant == FDSR_VARIANT_SR3;
  h->attn_blocks = c.variant != FDSR_VARIANT_FASTDIFFSR;
  h->plain_out = c.variant != FDSR_VARIANT_FASTDIFFSR;
  if (h->sr3) h->w_freq = add_weight(h, "time_mlp.0.inv_freq", {ic / 2}, true);   // registered buffer, ddpm_modules/unet.py:27
  b.embedding_mlp(h->sr3 ? "time_mlp" : "noise_level_mlp", 1, 3, ic, ic * 4, ic);
  int now_res = c.image_size;
  auto attn_here = [&]() { return h->attn_blocks && b.attn_res_has(now_res); };
  b.input_tensor();

  // One ResnetBlocWithAttn: consumes `cur` (concatenated with `skip` on the up path) and leaves its output there.
  // The schema order must follow torch's state_dict(): per module, registration order.  The reference registers res_block
  // (noise_func, block1, block2, res_conv), then conv, then attn or ca, sa.
  int cur = -1, curC = 0;
  auto res_block = [&](const std::string& p, Feat skip, int Cout, bool with_attn) -> int {
    const Src x = {cur, curC, skip.t, skip.C};
    const int Cin = x.C0 + x.C1;
    if (int rc = b.check_block_channels(p, x, Cout)) return rc;
    const std::string r = p + ".res_block";
    const int temb = b.embedding_rows(h->sr3 ? r + ".mlp.1" : r + ".noise_func.noise_func.0", Cout, ic);   // SR3: Sequential(Swish, Linear)
    const Norm n1 = b.norm_weights(r + ".block1.block.0", Cin);
    const ConvW w1 = b.conv_weights(r + ".block1.block.3", CONV3_S1, x.C0, x.C1, Cout);
    ResTail t;
    t.conv2 = r + ".block2";
    t.fill = r + ".res_conv";
    t.out = with_attn ? r : p;
    t.rider = true;
    t.n2 = b.norm_weights(r + ".block2.block.0", Cout);
    t.w2 = b.conv_weights(r + ".block2.block.3", CONV3_S1, Cout, 0, Cout);
    if (Cin != Cout) t.wfill = b.conv_weights(r + ".res_conv", CONV1, x.C0, x.C1, Cout);
    else if (x.C1) return fail(h, FDSR_E_INVALID, "%s: identity residual over a concatenated input is not supported", p.c_str());
    if (!h->attn_blocks) {
      add_weight(h, p + ".conv.weight", {Cout, Cout, 1, 1}, false);   // dead layer, unet.py:212
      add_weight(h, p + ".conv.bias", {Cout}, false);
    }

    // block1: GN -> Swish -> conv3x3, + noise shift
    const int slot1 = b.gn(r + ".block1.gn", x, n1);
    const int h1 = new_tensor(h, Cout, b.lvl, r + ".block1");
    Op& k1 = b.conv(r + ".block1", CONV3_S1, x, Cout, b.lvl, b.lvl, w1, h1);
    PlanBuilder::normed(k1, slot1, n1);
    k1.temb_off = temb;
    const int out = b.res_tail(t, x, x.x0, h1, Cout);
    cur = out;
    curC = Cout;
    if (with_attn && h->attn_blocks) {
      if (Cout % 32) return fail(h, FDSR_E_INVALID, "SelfAttention needs channels divisible by 32");
      cur = b.attention(SELF_ATTENTION, p + ".attn", p, out, Cout);
      h->tensors[out].name = r;   // the block output proper is the attention output
    } else if (with_attn) {
      if (Cout % 16) return fail(h, FDSR_E_INVALID, "CLAM needs channels divisible by 16");
      int f1 = add_weight(h, p + ".ca.fc1.weight", {Cout / 16, Cout, 1, 1}, true);
      int f2 = add_weight(h, p + ".ca.fc2.weight", {Cout, Cout / 16, 1, 1}, true);
      int s7 = add_weight(h, p + ".sa.conv1.weight", {1, 2, 7, 7}, true);
      Op ca; ca.kind = Op::CLAM; ca.name = p + ".ca"; ca.src0 = out; ca.C0 = Cout; ca.lvl_in = b.lvl; ca.fc1 = f1; ca.fc2 = f2;
      h->ops.push_back(ca);
      Op sa; sa.kind = Op::SLAM; sa.name = p + ".sa"; sa.src0 = out; sa.C0 = Cout; sa.lvl_in = b.lvl; sa.w = s7;
      sa.dst = new_tensor(h, Cout, b.lvl, p);
      h->ops.push_back(sa);
      h->Cmid = std::max(h->Cmid, Cout);
      cur = sa.dst;
    }
    return FDSR_OK;
  };
  const Feat none = {-1, 0};

  // downs
  std::vector<Feat> feats;
  cur = b.plain_conv("downs.0", "downs.0", CONV3_S1, h->t_in, h->CP, ic, 0, 0, c.in_channel);
  curC = ic;
  feats.push_back({cur, curC});
  int idx = 1;
  for (int ind = 0; ind < c.n_mults; ++ind) {
    const bool is_last = ind == c.n_mults - 1;
    const int cm = ic * c.channel_mults[ind];
    for (int rb = 0; rb < c.res_blocks; ++rb) {
      if (int rc = res_block("downs." + std::to_string(idx++), none, cm, attn_here())) return rc;
      feats.push_back({cur, curC});
    }
    if (!is_last) {
      const std::string p = "downs." + std::to_string(idx);
      cur = b.plain_conv(p + ".conv", p, CONV3_S2, cur, curC, curC, b.lvl, b.lvl + 1);
      ++b.lvl; ++idx;
      now_res /= 2;
      feats.push_back({cur, curC});
    }
  }
  // mid
  if (int rc = res_block("mid.0", none, curC, true)) return rc;
  if (int rc = res_block("mid.1", none, curC, false)) return rc;
  // ups
  idx = 0;
  for (int ind = c.n_mults - 1; ind >= 0; --ind) {
    const bool is_last = ind < 1;
    const int cm = ic * c.channel_mults[ind];
    for (int rb = 0; rb < c.res_blocks + 1; ++rb) {
      const Feat skip = feats.back();
      feats.pop_back();
      if (int rc = res_block("ups." + std::to_string(idx++), skip, cm, attn_here())) return rc;   // cat((x, skip)) unet.py:319
    }
    if (!is_last) {
      const std::string p = "ups." + std::to_string(idx);
      cur = b.plain_conv(p + ".conv", p, CONV3_UP, cur, curC, curC, b.lvl, b.lvl - 1);
      --b.lvl; ++idx;
      now_res *= 2;
    }
  }
  // final_conv = Block(pre, out_channel)
  if (curC % G) return fail(h, FDSR_E_INVALID, "final_conv: channels not divisible by norm_groups");
  b.output_head("final_conv", "final_conv.block.0", "final_conv.block.3", cur, curC);
  return b.finish(ic, ic / 2);
}

// Plan of the GDP sibling: model/gdp_modules/unet.py:530-800 (the guided-diffusion UNet as define_G instantiates it:
// use_scale_shift_norm, resblock_updown, num_head_channels = 64, conv_resample).  cfg.inner_channel carries
// model_channels (the reference's constructor ignores `inner_channel` and keeps its default 128), cfg.attn_res the
// attention_resolutions (downsample rates at which AttentionBlocks sit; reference default (32, 16, 8)).
int build_plan_gdp(fdsr_handle h) {
  const fdsr_config& c = h->cfg;
  const int mc = c.inner_channel, ted = 4 * mc;
  PlanBuilder b{h};
  if (int rc = b.check_config("model_channels")) return rc;   // build_plan made the same checks under the config field's name
  h->gdp = true;
  h->attn_blocks = true;
  h->plain_out = true;
  b.embedding_mlp("time_embed", 0, 2, mc, ted, ted);
  b.input_tensor();

  // POOL2 / UP2X of x into a temporary at lvl_out; gn_slot >= 0: of the normalised, activated x
  auto resample = [&](Op::Kind kind, const std::string& name, int x, int C, int lvl_out, int gn_slot) -> int {
    Op r; r.kind = kind; r.name = name; r.src0 = x; r.C0 = C; r.lvl_in = b.lvl; r.lvl_out = lvl_out; r.gn_slot = gn_slot;
    r.dst = new_tensor(h, C, lvl_out, "");
    h->ops.push_back(r);
    return r.dst;
  };
  enum Mode { PLAIN, DOWN, UP };
  // ResBlock (gdp_modules/unet.py:276-390): out = skip(x') + conv(dropout(silu(norm(h) * (1 + s) + t))),
  // h = conv(resample(silu(norm(x)))), (s, t) = Linear(silu(emb)); x' = resample(x)
  // Consumes `cur` (concatenated with `skip` in the output blocks) and leaves its output there, like attn_block.
  int cur = -1, ch = mc * c.channel_mults[0];
  auto res_block = [&](const std::string& p, Feat skip, int Cout, Mode mode) -> int {
    const Src x = {cur, ch, skip.t, skip.C};
    const int Cin = x.C0 + x.C1;
    if (int rc = b.check_block_channels(p, x, Cout)) return rc;
    if (mode != PLAIN && (x.C1 || Cin != Cout)) return fail(h, FDSR_E_INVALID, "%s: up/down ResBlocks keep the channel count", p.c_str());
    const Norm n1 = b.norm_weights(p + ".in_layers.0", Cin);
    const ConvW w1 = b.conv_weights(p + ".in_layers.2", mode == UP ? CONV3_UP : CONV3_S1, x.C0, x.C1, Cout);
    ResTail t;
    t.conv2 = p + ".out_layers";
    t.fill = p + ".skip_connection";
    t.out = p;
    t.film_off = b.embedding_rows(p + ".emb_layers.1", 2 * Cout, ted);
    t.n2 = b.norm_weights(p + ".out_layers.0", Cout);
    t.w2 = b.conv_weights(p + ".out_layers.3", CONV3_S1, Cout, 0, Cout);
    if (Cin != Cout) t.wfill = b.conv_weights(p + ".skip_connection", CONV1, x.C0, x.C1, Cout);
    else if (x.C1) return fail(h, FDSR_E_INVALID, "%s: identity skip over a concatenated input is not supported", p.c_str());

    const int slot1 = b.gn(p + ".in_layers.gn", x, n1);
    const int lvl_in = b.lvl, lvl_out = mode == DOWN ? lvl_in + 1 : (mode == UP ? lvl_in - 1 : lvl_in);
    Src hsrc = x;
    int xres = x.x0;
    if (mode == DOWN) {   // avg_pool(silu(norm(x))) and avg_pool(x), materialised one level down
      const int ph = resample(Op::POOL2, p + ".h_upd", x.x0, Cin, lvl_out, slot1);
      xres = resample(Op::POOL2, p + ".x_upd", x.x0, Cin, lvl_out, -1);
      hsrc = {ph, Cin};
    } else if (mode == UP) {   // x' = nearest-x2(x)
      xres = resample(Op::UP2X, p + ".x_upd", x.x0, Cin, lvl_out, -1);
    }
    const int h1 = new_tensor(h, Cout, lvl_out, p + ".in_layers");
    // DOWN: conv of the pooled tensor, which is activated already: no GroupNorm prologue.
    // UP: conv over nearest-x2(silu(norm(x))): the upsample conv with the GroupNorm prologue, which the sub-pixel kernel does not have.
    Op& k1 = b.conv(p + ".in_layers", mode == UP ? CONV3_UP : CONV3_S1, hsrc, Cout, mode == DOWN ? lvl_out : lvl_in, lvl_out, w1, h1);
    if (mode != DOWN) PlanBuilder::normed(k1, slot1, n1);
    k1.force_generic = mode == UP;
    b.lvl = lvl_out;
    cur = b.res_tail(t, x, xres, h1, Cout);
    ch = Cout;
    return FDSR_OK;
  };
  // AttentionBlock: heads of 64 channels
  auto attn_block = [&](const std::string& p) -> int {
    if (ch % 64) return fail(h, FDSR_E_INVALID, "%s: AttentionBlock needs channels divisible by num_head_channels = 64", p.c_str());
    cur = b.attention(ATTENTION_BLOCK, p, p, cur, ch);
    return FDSR_OK;
  };
  const Feat none = {-1, 0};

  std::vector<Feat> hs;
  int ds = 1, idx = 1;
  const int input_ch = ch;
  cur = b.plain_conv("input_blocks.0.0", "input_blocks.0", CONV3_S1, h->t_in, h->CP, ch, 0, 0, c.in_channel);
  hs.push_back({cur, ch});
  for (int level = 0; level < c.n_mults; ++level) {
    const int cm = mc * c.channel_mults[level];
    for (int rb = 0; rb < c.res_blocks; ++rb) {
      const std::string p = "input_blocks." + std::to_string(idx);
      if (int rc = res_block(p + ".0", none, cm, PLAIN)) return rc;
      if (b.attn_res_has(ds))
        if (int rc = attn_block(p + ".1")) return rc;
      h->tensors[cur].name = p;
      hs.push_back({cur, ch});
      ++idx;
    }
    if (level != c.n_mults - 1) {
      const std::string p = "input_blocks." + std::to_string(idx);
      if (int rc = res_block(p + ".0", none, ch, DOWN)) return rc;
      h->tensors[cur].name = p;
      hs.push_back({cur, ch});
      ds *= 2; ++idx;
    }
  }
  if (int rc = res_block("middle_block.0", none, ch, PLAIN)) return rc;
  if (int rc = attn_block("middle_block.1")) return rc;
  if (int rc = res_block("middle_block.2", none, ch, PLAIN)) return rc;
  h->tensors[cur].name = "middle_block";
  idx = 0;
  for (int level = c.n_mults - 1; level >= 0; --level) {
    const int cm = mc * c.channel_mults[level];
    for (int i = 0; i < c.res_blocks + 1; ++i) {
      const Feat skip = hs.back();
      hs.pop_back();
      const std::string p = "output_blocks." + std::to_string(idx);
      int sub = 0;
      if (int rc = res_block(p + "." + std::to_string(sub++), skip, cm, PLAIN)) return rc;   // th.cat([h, hs.pop()], dim=1)
      if (b.attn_res_has(ds))
        if (int rc = attn_block(p + "." + std::to_string(sub++))) return rc;
      if (level && i == c.res_blocks) {
        if (int rc = res_block(p + "." + std::to_string(sub++), none, ch, UP)) return rc;
        ds /= 2;
      }
      h->tensors[cur].name = p;
      ++idx;
    }
  }
  // out = GroupNorm -> SiLU -> conv(input_ch -> out_channel)
  if (ch != input_ch) return fail(h, FDSR_E_INVALID, "internal: GDP output width");
  b.output_head("out", "out.0", "out.2", cur, ch);
  return b.finish(ted, mc / 2);
}

}  // namespace

namespace fdsr_int {

// Build the static plan (ops, tensors, weight schema) of h->cfg.
int build_plan(fdsr_handle h) {
  const fdsr_config& c = h->cfg;
  PlanBuilder b{h};
  if (int rc = b.check_config("inner_channel")) return rc;
  if (c.variant < 0 || c.variant > FDSR_VARIANT_GDP) return fail(h, FDSR_E_INVALID, "unknown variant %d", c.variant);
  return c.variant == FDSR_VARIANT_GDP ? build_plan_gdp(h) : build_plan_unet(h);
}

}  // namespace fdsr_int
