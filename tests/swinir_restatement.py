"""SwinIR restated in plain torch from the architecture (not a test module; tests import it): the network that
fastdiffsr_amd.swinir runs on the device, written functionally over a dict of weights under the reference's state_dict
names, runnable in fp32 and fp64 on the CPU or, for timing, on a GPU.

    taps = swinir_forward(weights, cfg, x, dtype=torch.float64)

returns every named tap of swinir.arch.tap_names(cfg) as NCHW at the padded size, and 'out'.  `broken` switches one piece to
a plausible wrong form, so that a test can show that its tolerance would catch it:
    'no_mask'          shifted windows attend across the seam of the rolled image
    'bias_transposed'  the relative-position bias is indexed (key, query) for (query, key)
    'roll_reversed'    the cyclic shift goes by +shift before the windows and by -shift after them
    'gelu_tanh'        the tanh form of GELU in place of the erf form
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BROKEN = ('no_mask', 'bias_transposed', 'roll_reversed', 'gelu_tanh')
MEAN = (0.4488, 0.4371, 0.4040)
WS = 8
GOLDEN_CAP = 8192

# ---- the cases of tests/golden/swinir.npz (tools/make_swinir_golden.py runs the reference on them) ----
SEED = 11                                  # of synth.synth_swinir
SMALL = dict(img_size=64, embed_dim=36, depths=[2, 2], num_heads=[6, 6], window_size=8, mlp_ratio=2.)
FULL = dict(img_size=64, embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, window_size=8, mlp_ratio=2.)
# name: (configuration, upscale, (H, W) of the LR input, taps recorded); the input is case_input(name, 1, H, W)
CASES = {
    's4_8x8': (SMALL, 4, (8, 8), True),
    's4_16x24': (SMALL, 4, (16, 24), True),
    's4_12x20': (SMALL, 4, (12, 20), False),
    's2_8x8': (SMALL, 2, (8, 8), False),
    's3_8x8': (SMALL, 3, (8, 8), False),
    'full_16x16': (FULL, 4, (16, 16), False),
}


def case_input(name, b, h, w):
    """[b, 3, h, w] in [0, 1): the input of a case, from the case's name."""
    return torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(zlib.crc32(name.encode())))


def recorded_taps(names):
    """Of arch.tap_names, the taps a case with taps records and the tests check: every one but the blocks after layer 0's first two."""
    return [t for t in names if '.blocks.' not in t or t.startswith(('layers.0.blocks.0.', 'layers.0.blocks.1.'))]


def sample_index(key, numel, cap=GOLDEN_CAP):
    """tests/golden/swinir.npz keeps a tensor of more than `cap` elements as a fixed sample of its flat elements (the file
    stays under the size limit for fixtures): the sorted flat indices of that sample, or None for a tensor kept whole."""
    if numel <= cap:
        return None
    return np.sort(np.random.default_rng(zlib.crc32(key.encode())).choice(numel, cap, replace=False))


def sampled(key, t):
    """The elements of tensor / array t that the golden file holds under `key`, flat."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    idx = sample_index(key, a.size)
    return a.reshape(-1) if idx is None else a.reshape(-1)[idx]


def _windows(t):
    """[B, H, W, C] -> [B * nW, 64, C], windows row-major, tokens row-major inside a window."""
    b, h, w, c = t.shape
    return t.reshape(b, h // WS, WS, w // WS, WS, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, WS * WS, c)


def _unwindows(t, b, h, w):
    c = t.shape[-1]
    return t.reshape(b, h // WS, w // WS, WS, WS, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)


@functools.lru_cache(maxsize=None)
def _pair_index(device):
    """[64, 64]: the bias-table row of (query i, key j): their offset (dy, dx), each in [-7, 7], as a base-15 number."""
    y, x = torch.arange(WS * WS, device=device) // WS, torch.arange(WS * WS, device=device) % WS
    return (y[:, None] - y[None, :] + WS - 1) * (2 * WS - 1) + (x[:, None] - x[None, :] + WS - 1)


@functools.lru_cache(maxsize=None)
def _seam_mask(h, w, shift, dtype, device):
    """[nW, 64, 64]: -100 where two tokens of a window of the rolled image come from different sides of a seam.  Along each
    axis the last `shift` rows wrapped around, the WS - shift rows before them share windows with those, the rest never do.
    A function of the size alone, kept per size as the reference keeps its attn_mask buffer."""
    def side(n):
        i = torch.arange(n, device=device)
        return (i >= n - WS).long() + (i >= n - shift).long()
    region = (side(h)[:, None] * 3 + side(w)[None, :]).reshape(1, h, w, 1)
    r = _windows(region).squeeze(-1)
    return torch.where(r[:, :, None] != r[:, None, :], -100.0, 0.0).to(dtype)


def _layer_norm(t, wt, name):
    return F.layer_norm(t, (t.shape[-1],), wt[name + '.weight'], wt[name + '.bias'], 1e-5)


def _block(t, wt, name, heads, shift, broken):
    b, h, w, c = t.shape
    hd = c // heads
    y = _layer_norm(t, wt, name + '.norm1')
    fwd = -shift if broken != 'roll_reversed' else shift
    if shift:
        y = torch.roll(y, (fwd, fwd), (1, 2))
    win = _windows(y)                                                        # [n, 64, C]
    qkv = F.linear(win, wt[name + '.attn.qkv.weight'], wt[name + '.attn.qkv.bias'])
    q, k, v = qkv.reshape(-1, WS * WS, 3, heads, hd).permute(2, 0, 3, 1, 4)  # each [n, heads, 64, hd]
    idx = _pair_index(t.device)
    if broken == 'bias_transposed':
        idx = idx.t()
    bias = wt[name + '.attn.relative_position_bias_table'][idx.reshape(-1)].reshape(WS * WS, WS * WS, heads).permute(2, 0, 1)
    s = (q * hd ** -0.5) @ k.transpose(-2, -1) + bias
    if shift and broken != 'no_mask':
        m = _seam_mask(h, w, shift, t.dtype, t.device)
        s = (s.reshape(b, -1, heads, WS * WS, WS * WS) + m[None, :, None]).reshape(-1, heads, WS * WS, WS * WS)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(-1, WS * WS, c)
    o = F.linear(o, wt[name + '.attn.proj.weight'], wt[name + '.attn.proj.bias'])
    o = _unwindows(o, b, h, w)
    if shift:
        o = torch.roll(o, (-fwd, -fwd), (1, 2))
    t = t + o
    after_attn = t
    y = F.linear(_layer_norm(t, wt, name + '.norm2'), wt[name + '.mlp.fc1.weight'], wt[name + '.mlp.fc1.bias'])
    y = F.gelu(y, approximate='tanh' if broken == 'gelu_tanh' else 'none')
    return after_attn, t + F.linear(y, wt[name + '.mlp.fc2.weight'], wt[name + '.mlp.fc2.bias'])


def _conv(t, wt, name):
    """3x3, zero halo; t is NHWC."""
    return F.conv2d(t.permute(0, 3, 1, 2), wt[name + '.weight'], wt[name + '.bias'], padding=1).permute(0, 2, 3, 1)


def swinir_forward(weights, cfg, x, dtype=torch.float64, broken=None):
    assert broken is None or broken in BROKEN
    wt = {k: torch.as_tensor(v).to(device=x.device, dtype=dtype) for k, v in weights.items()}
    taps = {}

    def tap(name, t):
        taps[name] = t.permute(0, 3, 1, 2).contiguous()

    x = x.to(dtype)
    h0, w0 = x.shape[2:]
    x = F.pad(x, (0, -w0 % WS, 0, -h0 % WS), 'reflect')
    mean = torch.tensor(MEAN, dtype=dtype, device=x.device).reshape(1, 3, 1, 1)
    t = ((x - mean) * cfg.img_range).permute(0, 2, 3, 1)
    first = _conv(t, wt, 'conv_first')
    tap('conv_first', first)
    t = _layer_norm(first, wt, 'patch_embed.norm') if cfg.patch_norm else first
    tap('patch_embed.norm', t)
    for i, (depth, heads) in enumerate(zip(cfg.depths, cfg.num_heads)):
        group_in = t
        for j in range(depth):
            a, t = _block(t, wt, f'layers.{i}.residual_group.blocks.{j}', heads, cfg.window_size // 2 if j % 2 else 0, broken)
            tap(f'layers.{i}.blocks.{j}.attn', a)
            tap(f'layers.{i}.blocks.{j}.mlp', t)
        t = _conv(t, wt, f'layers.{i}.conv') + group_in
        tap(f'layers.{i}', t)
    t = _conv(_layer_norm(t, wt, 'norm'), wt, 'conv_after_body') + first
    tap('conv_after_body', t)
    t = F.leaky_relu(_conv(t, wt, 'conv_before_upsample.0'), 0.01)
    for k, (idx, r) in enumerate(cfg.upsample_convs()):
        t = F.pixel_shuffle(_conv(t, wt, f'upsample.{idx}').permute(0, 3, 1, 2), r).permute(0, 2, 3, 1)
        tap(f'upsample.{k}', t)
    out = _conv(t, wt, 'conv_last').permute(0, 3, 1, 2) / cfg.img_range + mean
    taps['out'] = out[:, :, :h0 * cfg.upscale, :w0 * cfg.upscale].contiguous()
    return taps


def save_img1(x):
    """[3, H, W] float tensor -> HWC uint8, the arithmetic of the reference's srutils.save_img1: times 255, clamp, truncate."""
    return (x * 255.0).clamp(0, 255).detach().cpu().numpy().transpose(1, 2, 0).astype('uint8')
