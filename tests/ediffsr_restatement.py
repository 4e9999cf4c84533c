"""Plain-torch CPU restatement of EDiffSR's ConditionalNAFNet.forward and of the IR-SDE reverse loops, written from
EDiffSR/codes (DenoisingNAFNet_arch.py, module_util.py, utils/sde_utils.py): functional, dtype-generic, no hooks.

Two things are pinned on purpose:
  * LayerNorm's eps is 1e-5 in EVERY dtype.  The reference picks `1e-5 if x.dtype == float32 else 1e-3`, so a `.double()` copy of
    its module computes a different function; an fp64 yardstick must not.
  * the sinusoidal embedding is formed in fp32 (the reference's time is an int or an fp32 tensor) and cast afterwards.
tests/golden/ediffsr.npz (tools/make_ediffsr_golden.py) pins this file to the reference's own modules in fp32."""
import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-5


def layer_norm(x, g):
    var = torch.var(x, dim=1, unbiased=False, keepdim=True)
    mean = torch.mean(x, dim=1, keepdim=True)
    return (x - mean) * (var + LN_EPS).rsqrt() * g


def simple_gate(x):
    a, b = x.chunk(2, dim=1)
    return a * b


def sinusoidal(time, dim):
    half = dim // 2
    emb = math.log(10000) / (half - 1)
    emb = torch.exp(torch.arange(half, device=time.device) * -emb)     # fp32, as the reference
    emb = time[:, None] * emb[None, :]
    return torch.cat((emb.sin(), emb.cos()), dim=-1)


def naf_block(sd, p, x, t):
    inp = x
    temb = F.linear(simple_gate(t), sd[p + '.mlp.1.weight'], sd[p + '.mlp.1.bias'])[:, :, None, None]
    shift_att, scale_att, shift_ffn, scale_ffn = temb.chunk(4, dim=1)
    x = layer_norm(inp, sd[p + '.norm1.g'])
    x = x * (scale_att + 1) + shift_att
    x = F.conv2d(x, sd[p + '.conv1.weight'], sd[p + '.conv1.bias'])
    x = F.conv2d(x, sd[p + '.conv2.weight'], sd[p + '.conv2.bias'], padding=1, groups=x.shape[1])
    x = simple_gate(x)
    x = x * F.conv2d(x.mean(dim=(2, 3), keepdim=True), sd[p + '.sca.1.weight'], sd[p + '.sca.1.bias'])
    x = F.conv2d(x, sd[p + '.conv3.weight'], sd[p + '.conv3.bias'])
    y = inp + x * sd[p + '.beta']
    x = layer_norm(y, sd[p + '.norm2.g'])
    x = x * (scale_ffn + 1) + shift_ffn
    x = F.conv2d(x, sd[p + '.conv4.weight'], sd[p + '.conv4.bias'])
    x = simple_gate(x)
    x = F.conv2d(x, sd[p + '.conv5.weight'], sd[p + '.conv5.bias'])
    return y + x * sd[p + '.gamma']


def rcab(sd, p, x):
    r = F.conv2d(x, sd[p + '.rcab.0.weight'], sd[p + '.rcab.0.bias'], padding=1)
    r = F.conv2d(F.relu(r), sd[p + '.rcab.2.weight'], sd[p + '.rcab.2.bias'], padding=1)
    a = r.mean(dim=(2, 3), keepdim=True)
    a = F.relu(F.conv2d(a, sd[p + '.rcab.3.attention.1.weight'], sd[p + '.rcab.3.attention.1.bias']))
    a = torch.sigmoid(F.conv2d(a, sd[p + '.rcab.3.attention.3.weight'], sd[p + '.rcab.3.attention.3.bias']))
    return r * a + x


def count_blocks(sd, prefix):
    n = 0
    while (prefix % n) + '.beta' in sd:
        n += 1
    return n


def forward(sd, inp, cond, time, taps=None):
    """sd: the state dict in the compute dtype; inp, cond [B,3,H,W] in that dtype; time: int, float or tensor [1] / [B].
    taps: a dict that receives every named intermediate (arch.tap_names), or None."""
    dtype = inp.dtype
    width = sd['intro.weight'].shape[0]
    levels = 0
    while 'downs.%d.weight' % levels in sd:
        levels += 1
    if isinstance(time, (int, float)):
        time = torch.tensor([time])
    time = time.to(torch.float32) if time.dtype != torch.float32 else time

    def tap(name, v):
        if taps is not None:
            taps[name] = v
        return v

    x = torch.cat([inp - cond, cond], dim=1)
    t = sinusoidal(time, width).to(dtype)
    t = F.linear(t, sd['time_mlp.1.weight'], sd['time_mlp.1.bias'])
    t = F.linear(simple_gate(t), sd['time_mlp.3.weight'], sd['time_mlp.3.bias'])
    B, C, H, W = x.shape
    pad = 2 ** levels
    x = F.pad(x, (0, (pad - W % pad) % pad, 0, (pad - H % pad) % pad))
    x = tap('intro', F.conv2d(x, sd['intro.weight'], sd['intro.bias'], padding=1))
    x = tap('enhance', x + rcab(sd, 'enhance', x))
    encs = []
    for i in range(levels):
        for j in range(count_blocks(sd, 'encoders.%d.%%d' % i)):
            x = tap('encoders.%d.%d' % (i, j), naf_block(sd, 'encoders.%d.%d' % (i, j), x, t))
        encs.append(x)
        x = tap('downs.%d' % i, F.conv2d(x, sd['downs.%d.weight' % i], sd['downs.%d.bias' % i], stride=2))
    for j in range(count_blocks(sd, 'middle_blks.%d')):
        x = tap('middle_blks.%d' % j, naf_block(sd, 'middle_blks.%d' % j, x, t))
    for i, skip in enumerate(encs[::-1]):
        x = F.pixel_shuffle(F.conv2d(x, sd['ups.%d.0.weight' % i]), 2)
        x = tap('ups.%d' % i, x + skip)
        for j in range(count_blocks(sd, 'decoders.%d.%%d' % i)):
            x = tap('decoders.%d.%d' % (i, j), naf_block(sd, 'decoders.%d.%d' % (i, j), x, t))
    x = tap('ending', F.conv2d(x, sd['ending.weight'], sd['ending.bias'], padding=1))
    return x[..., :H, :W]


def reverse_loop(sd, tables, state, mu, noise=None, ode=False, trajectory=None):
    """IRSDE.reverse_sde (noise [T,B,3,H,W]: plane k is the randn_like of step t = T - k) / reverse_ode, with the tables
    (thetas, sigmas, sigma_bars, dt) of sde.IRSDE cast to the compute dtype.  trajectory: a list that receives x after every step."""
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


def cast_tables(sde, dtype):
    return (sde.thetas.to(dtype), sde.sigmas.to(dtype), sde.sigma_bars.to(dtype), sde.dt.to(dtype))


def cast_sd(sd, dtype):
    return {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
