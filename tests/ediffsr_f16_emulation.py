"""CPU emulation of the NAFNet's f16 storage mode (include/fdsr.h: fdsr_nafnet_set_storage) on top of tests/ediffsr_restatement.py:
the yardstick of the mode's arithmetic, independent of the device code.  Its own naf_block / forward / reverse_loop, with the
header's rounding points:
  * a dense convolution rounds its input (after LN + FiLM / the SCA multiply) and its weight to f16, takes the products of those
    f16 values in fp64 and rounds the sum to fp32; bias and epilogue follow in fp32
  * every tensor the network stores between kernels is rounded to f16 once -- y and out after the residual, the depthwise output
    after the gate, the ups after PixelShuffle + skip -- and read back widened; the network input and ending's output stay fp32
  * the SCA pool's means come from the gate values before their rounding; the RCAB's pool reads the stored tensor
  * LayerNorm, FiLM, the depthwise taps, gates, SCA / CA and the time path are the restatement's fp32
A value beyond +-65504 is clamped before the rounding.  (The device scales a weight by a power of two before rounding it, which is
exact.)"""
import math

import torch
import torch.nn.functional as F

import ediffsr_restatement as R

F16_MAX = 65504.0


def rnd(v):
    """fp32 tensor -> fp32 tensor of f16 values: clamp to +-65504, round to nearest even"""
    return v.float().clamp(-F16_MAX, F16_MAX).half().float()


def conv_h(x, w, b=None, stride=1, padding=0):
    """one f16 product per term, summed in fp64, rounded to fp32; bias in fp32"""
    y = F.conv2d(rnd(x).double(), rnd(w).double(), None, stride, padding).float()
    return y if b is None else y + b.float().view(1, -1, 1, 1)


def naf_block(sd, p, x, t):
    inp = x
    temb = F.linear(R.simple_gate(t), sd[p + '.mlp.1.weight'], sd[p + '.mlp.1.bias'])[:, :, None, None]
    shift_att, scale_att, shift_ffn, scale_ffn = temb.chunk(4, dim=1)
    x = R.layer_norm(inp, sd[p + '.norm1.g']) * (scale_att + 1) + shift_att
    x = rnd(conv_h(x, sd[p + '.conv1.weight'], sd[p + '.conv1.bias']))
    g = R.simple_gate(F.conv2d(x, sd[p + '.conv2.weight'], sd[p + '.conv2.bias'], padding=1, groups=x.shape[1]))
    sca = F.conv2d(g.mean(dim=(2, 3), keepdim=True), sd[p + '.sca.1.weight'], sd[p + '.sca.1.bias'])   # the unrounded gate values
    x = conv_h(rnd(g) * sca, sd[p + '.conv3.weight'], sd[p + '.conv3.bias'])
    y = rnd(inp + x * sd[p + '.beta'])
    x = R.layer_norm(y, sd[p + '.norm2.g']) * (scale_ffn + 1) + shift_ffn
    x = rnd(R.simple_gate(conv_h(x, sd[p + '.conv4.weight'], sd[p + '.conv4.bias'])))
    return rnd(y + conv_h(x, sd[p + '.conv5.weight'], sd[p + '.conv5.bias']) * sd[p + '.gamma'])


def enhance(sd, x):
    """x + enhance(x) with R.rcab's arithmetic and the two stored convolution outputs"""
    p = 'enhance'
    r = rnd(F.relu(conv_h(x, sd[p + '.rcab.0.weight'], sd[p + '.rcab.0.bias'], padding=1)))
    r = rnd(conv_h(r, sd[p + '.rcab.2.weight'], sd[p + '.rcab.2.bias'], padding=1))
    a = r.mean(dim=(2, 3), keepdim=True)
    a = F.relu(F.conv2d(a, sd[p + '.rcab.3.attention.1.weight'], sd[p + '.rcab.3.attention.1.bias']))
    a = torch.sigmoid(F.conv2d(a, sd[p + '.rcab.3.attention.3.weight'], sd[p + '.rcab.3.attention.3.bias']))
    return rnd(x + (r * a + x))


def forward(sd, inp, cond, time, taps=None):
    """ediffsr_restatement.forward in fp32 with the storage mode's roundings; taps as there"""
    with torch.no_grad():
        sd = R.cast_sd(sd, torch.float32)
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
                taps[name] = v
            return v

        x = torch.cat([inp - cond, cond], dim=1)
        t = R.sinusoidal(time, width)
        t = F.linear(t, sd['time_mlp.1.weight'], sd['time_mlp.1.bias'])
        t = F.linear(R.simple_gate(t), sd['time_mlp.3.weight'], sd['time_mlp.3.bias'])
        B, C, H, W = x.shape
        pad = 2 ** levels
        x = F.pad(x, (0, (pad - W % pad) % pad, 0, (pad - H % pad) % pad))
        x = tap('intro', rnd(conv_h(x, sd['intro.weight'], sd['intro.bias'], padding=1)))
        x = tap('enhance', enhance(sd, x))
        encs = []
        for i in range(levels):
            for j in range(R.count_blocks(sd, 'encoders.%d.%%d' % i)):
                x = tap('encoders.%d.%d' % (i, j), naf_block(sd, 'encoders.%d.%d' % (i, j), x, t))
            encs.append(x)
            x = tap('downs.%d' % i, rnd(conv_h(x, sd['downs.%d.weight' % i], sd['downs.%d.bias' % i], stride=2)))
        for j in range(R.count_blocks(sd, 'middle_blks.%d')):
            x = tap('middle_blks.%d' % j, naf_block(sd, 'middle_blks.%d' % j, x, t))
        for i, skip in enumerate(encs[::-1]):
            x = F.pixel_shuffle(conv_h(x, sd['ups.%d.0.weight' % i]), 2)
            x = tap('ups.%d' % i, rnd(x + skip))
            for j in range(R.count_blocks(sd, 'decoders.%d.%%d' % i)):
                x = tap('decoders.%d.%d' % (i, j), naf_block(sd, 'decoders.%d.%d' % (i, j), x, t))
        x = tap('ending', conv_h(x, sd['ending.weight'], sd['ending.bias'], padding=1))   # fp32 eps
        return x[..., :H, :W]


def reverse_loop(sd, tables, state, mu, noise=None, ode=False, trajectory=None):
    """ediffsr_restatement.reverse_loop around this file's forward: the SDE state, mu, the noise and the step stay fp32"""
    thetas, sigmas, sigma_bars, dt = tables
    T = thetas.numel() - 1
    x = state.clone()
    for k, t in enumerate(reversed(range(1, T + 1))):
        score = -forward(sd, x, mu, t) / sigma_bars[t]
        if ode:
            x = x - (thetas[t] * (mu - x) - 0.5 * sigmas[t] ** 2 * score) * dt
        else:
            x = x - (thetas[t] * (mu - x) - sigmas[t] ** 2 * score) * dt - sigmas[t] * (noise[k] * math.sqrt(dt))
        if trajectory is not None:
            trajectory.append(x)
    return x
