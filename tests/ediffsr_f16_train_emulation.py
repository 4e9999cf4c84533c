"""CPU emulation of training under f16 activation storage (include/fdsr.h: fdsr_nafnet_set_train_storage): the differentiable twin
of tests/ediffsr_f16_emulation.py.  The forward has that file's rounding points and values; the backward follows the header's
contract, independent of the device code:
  * a rounding passes its gradient straight through: ste(v) has rnd(v)'s value and v's gradient
  * a dense convolution (conv_t): the forward of conv_h (f16 input and weight, products summed in fp64, fp32 result); d input from the
    fp32 master weight, not the rounded one; d weight from the staged input -- rounded to f16 as the forward staged it, except
    intro's fp32 network input, which the weight gradient reads un-rounded; both gradients summed in fp64 and rounded to fp32
  * d beta / d gamma multiply the fp32 convolution outputs the forward scaled (before any rounding)
  * what the backward can only form from stored values: conv4's gate backward multiplies by the stored (rounded) pair, SCA's weight
    gradient takes the pooled mean of the stored gate output, ReLU's mask is that of the stored output
  * LayerNorm, FiLM, the depthwise taps, gates, SCA / CA, the time path are fp32 autograd over the stored values; the loss head
    (tests/ediffsr_train_restatement.py's) is evaluated in fp64 on the fp32 prediction
Gradients are fp32 everywhere and no loss scaling is applied."""
import torch
import torch.nn.functional as F

import ediffsr_f16_emulation as E
import ediffsr_restatement as R
import ediffsr_train_restatement as TR

rnd = E.rnd


class _ValueOf(torch.autograd.Function):
    """value's value with carrier's gradient"""

    @staticmethod
    def forward(ctx, carrier, value):
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def with_value(carrier, value):
    return _ValueOf.apply(carrier, value.detach())


def ste(v):
    """the stored tensor: rounded to f16, the gradient passed straight through"""
    return with_value(v, rnd(v))


class _ConvT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, w, b, a_w, stride, padding):
        ctx.save_for_backward(w, rnd(a) if a_w is None else a_w)
        ctx.conf = (stride, padding, tuple(a.shape), b is not None)
        return E.conv_h(a, w, b, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        w, a_w = ctx.saved_tensors
        stride, padding, a_shape, has_b = ctx.conf
        d = dy.double()
        da = torch.nn.grad.conv2d_input(a_shape, w.double(), d, stride, padding).float() if ctx.needs_input_grad[0] else None
        dw = torch.nn.grad.conv2d_weight(a_w.double(), tuple(w.shape), d, stride, padding).float()
        db = d.sum(dim=(0, 2, 3)).float() if has_b else None
        return da, dw, db, None, None, None


def conv_t(a, w, b=None, stride=1, padding=0, a_w=None):
    return _ConvT.apply(a, w, b, a_w, stride, padding)


def naf_block(sd, p, x, t):
    inp = x
    temb = F.linear(R.simple_gate(t), sd[p + '.mlp.1.weight'], sd[p + '.mlp.1.bias'])[:, :, None, None]
    shift_att, scale_att, shift_ffn, scale_ffn = temb.chunk(4, dim=1)
    x = R.layer_norm(inp, sd[p + '.norm1.g']) * (scale_att + 1) + shift_att
    x = ste(conv_t(x, sd[p + '.conv1.weight'], sd[p + '.conv1.bias']))
    g = R.simple_gate(F.conv2d(x, sd[p + '.conv2.weight'], sd[p + '.conv2.bias'], padding=1, groups=x.shape[1]))
    t2 = ste(g)

    def sca_of(pooled):
        return F.conv2d(pooled, sd[p + '.sca.1.weight'], sd[p + '.sca.1.bias'])
    # the value from the unrounded gate values, the gradients (d W_sca among them) from the stored ones
    sca = with_value(sca_of(t2.mean(dim=(2, 3), keepdim=True)), sca_of(g.mean(dim=(2, 3), keepdim=True)))
    x = conv_t(t2 * sca, sd[p + '.conv3.weight'], sd[p + '.conv3.bias'])
    y = ste(inp + x * sd[p + '.beta'])
    x = R.layer_norm(y, sd[p + '.norm2.g']) * (scale_ffn + 1) + shift_ffn
    u = conv_t(x, sd[p + '.conv4.weight'], sd[p + '.conv4.bias'])
    g4 = with_value(R.simple_gate(ste(u)), rnd(R.simple_gate(u)))   # the product of the fp32 pair, the partners of the stored pair
    return ste(y + conv_t(g4, sd[p + '.conv5.weight'], sd[p + '.conv5.bias']) * sd[p + '.gamma'])


def enhance(sd, x):
    p = 'enhance'
    r = F.relu(ste(conv_t(x, sd[p + '.rcab.0.weight'], sd[p + '.rcab.0.bias'], padding=1)))
    r = ste(conv_t(r, sd[p + '.rcab.2.weight'], sd[p + '.rcab.2.bias'], padding=1))
    a = r.mean(dim=(2, 3), keepdim=True)
    a = F.relu(F.conv2d(a, sd[p + '.rcab.3.attention.1.weight'], sd[p + '.rcab.3.attention.1.bias']))
    a = torch.sigmoid(F.conv2d(a, sd[p + '.rcab.3.attention.3.weight'], sd[p + '.rcab.3.attention.3.bias']))
    return ste(x + (r * a + x))


def forward(sd, inp, cond, time, taps=None):
    """ediffsr_f16_emulation.forward's values, differentiable with respect to sd (fp32 leaves)"""
    inp, cond = inp.float(), cond.float()
    width = sd['intro.weight'].shape[0]
    levels = 0
    while 'downs.%d.weight' % levels in sd:
        levels += 1
    if isinstance(time, (int, float)):
        time = torch.tensor([time])
    time = time.to(torch.float32)

    def tap(name, v):
        if taps is not None:
            taps[name] = v.detach()
        return v

    x = torch.cat([inp - cond, cond], dim=1)
    t = R.sinusoidal(time, width)
    t = F.linear(t, sd['time_mlp.1.weight'], sd['time_mlp.1.bias'])
    t = F.linear(R.simple_gate(t), sd['time_mlp.3.weight'], sd['time_mlp.3.bias'])
    B, C, H, W = x.shape
    pad = 2 ** levels
    x = F.pad(x, (0, (pad - W % pad) % pad, 0, (pad - H % pad) % pad))
    x = tap('intro', ste(conv_t(x, sd['intro.weight'], sd['intro.bias'], padding=1, a_w=x)))
    x = tap('enhance', enhance(sd, x))
    encs = []
    for i in range(levels):
        for j in range(R.count_blocks(sd, 'encoders.%d.%%d' % i)):
            x = tap('encoders.%d.%d' % (i, j), naf_block(sd, 'encoders.%d.%d' % (i, j), x, t))
        encs.append(x)
        x = tap('downs.%d' % i, ste(conv_t(x, sd['downs.%d.weight' % i], sd['downs.%d.bias' % i], stride=2)))
    for j in range(R.count_blocks(sd, 'middle_blks.%d')):
        x = tap('middle_blks.%d' % j, naf_block(sd, 'middle_blks.%d' % j, x, t))
    for i, skip in enumerate(encs[::-1]):
        x = F.pixel_shuffle(conv_t(x, sd['ups.%d.0.weight' % i]), 2)
        x = tap('ups.%d' % i, ste(x + skip))
        for j in range(R.count_blocks(sd, 'decoders.%d.%%d' % i)):
            x = tap('decoders.%d.%d' % (i, j), naf_block(sd, 'decoders.%d.%d' % (i, j), x, t))
    x = tap('ending', conv_t(x, sd['ending.weight'], sd['ending.bias'], padding=1))   # fp32 eps
    return x[..., :H, :W]


def loss_and_grads(sd, tables64, state, mu, x0, timesteps, loss_type='l1', weight=1.0):
    """sd: fp32 tensors; tables64: ediffsr_train_restatement.cast_tables(sde, torch.float64).  The loss head of
    ediffsr_train_restatement.loss on the fp32 prediction, in fp64.  Returns (loss, {key: fp32 gradient})."""
    leaves = {k: torch.as_tensor(v).float().detach().clone().requires_grad_(True) for k, v in sd.items()}
    t = timesteps.reshape(-1, 1, 1, 1).long()
    noise = forward(leaves, state, mu, t.reshape(-1)).double()
    state, mu, x0 = state.double(), mu.double(), x0.double()
    score = -noise / tables64[2][t]
    expect = TR.reverse_sde_step_mean(tables64, state, mu, score, t)
    optimum = TR.reverse_optimum_step(tables64, state, x0, mu, t)
    val = weight * TR.matching_loss(expect, optimum, loss_type)
    keys = list(leaves)
    gs = torch.autograd.grad(val, [leaves[k] for k in keys], allow_unused=True)
    return val.detach(), {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(keys, gs)}


# ---- the gradient cases of the f16 training tests, and their references (computed once per session) ----
TEST_SETTING = dict(width=16, enc_blk_nums=[2, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
SHIPPED_SETTING = dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
EMPTY_SETTING = dict(width=16, enc_blk_nums=[1, 0], middle_blk_num=0, dec_blk_nums=[0, 1])
SDE = dict(max_sigma=50, T=100, schedule='cosine', eps=0.005)
CASES = {
    'a': (TEST_SETTING, 2, 36, 44, [1, 100], 'l1'),      # ragged padding
    'b': (TEST_SETTING, 3, 32, 32, [7, 50, 93], 'l2'),
    'd': (SHIPPED_SETTING, 2, 32, 32, [12, 88], 'l1'),
    'e': (EMPTY_SETTING, 2, 18, 26, [3, 64], 'l1'),      # empty block lists; pads to 20 x 28
}
BATCH_SEED = 31
_REFERENCES = {}


def batch(seed, b, h, w, t, sde):
    """tests/test_gpu_ediffsr_train.py's _batch"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(b, 3, h, w, generator=g)
    mu = (gt + 0.1 * torch.randn(b, 3, h, w, generator=g)).clamp(0, 1)
    ts = torch.tensor(t).reshape(b, 1, 1, 1).long()
    sde.set_mu(mu)
    state = torch.randn(b, 3, h, w, generator=g) * sde.sigma_bar(ts) + sde.mu_bar(gt, ts)
    return gt, mu, state.float(), ts


def reference(case):
    """For one of CASES, with synth_nafnet(0) weights and batch(BATCH_SEED): the emulation's and fp64 autograd's loss and gradients,
    and s[k] = max|g_emul[k] - g64[k]| per tensor."""
    if case not in _REFERENCES:
        from fastdiffsr_amd.ediffsr.sde import IRSDE
        from fastdiffsr_amd.synth import synth_nafnet
        setting, b, h, w, t, loss_type = CASES[case]
        sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **setting).items()}
        sde = IRSDE(device='cpu', **SDE)
        gt, mu, state, ts = batch(BATCH_SEED, b, h, w, t, sde)
        t64 = TR.cast_tables(sde, torch.float64)
        l64, g64 = TR.loss_and_grads(R.cast_sd(sd, torch.float64), t64, state.double(), mu.double(), gt.double(), ts, loss_type)
        le, ge = loss_and_grads(sd, t64, state, mu, gt, ts, loss_type)
        s = {k: float((ge[k].double() - g64[k]).abs().max()) for k in g64}
        _REFERENCES[case] = dict(l_emul=float(le), l64=float(l64), g_emul=ge, g64=g64, s=s, batch=(gt, mu, state, ts), loss_type=loss_type,
                                 setting=setting)
    return _REFERENCES[case]
