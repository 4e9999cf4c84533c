"""TransENet restated in plain torch from the architecture (not a test module; tests import it): the network that
fastdiffsr_amd.transenet runs on the device, written functionally over a dict of weights under the reference's state_dict
names, runnable in fp32 and fp64 on the CPU or, for timing, on a GPU.

    taps = transenet_forward(weights, cfg, x, dtype=torch.float64)

returns every named tap of transenet.arch.tap_names(cfg) as NCHW (a token tensor as [B, 512, h, w] over the grid of patches)
and 'out'.  The geometry is the input's: cfg.hr_patch_size is not consulted (the module checks it).  `broken` switches one
piece to a plausible wrong form, so that a test can show that its tolerance would catch it:
    'scale_dim_head'     the logit scale is dim_head ** -0.5 = 32^-0.5 in place of dim ** -0.5 = 512^-0.5
    'gelu_erf'           the erf form of GELU in place of the reference's own tanh form
    'decoder_order'      decoder1 runs first (1, 2, 3 in place of 3, 2, 1), each with its own stage's memory
    'memory_not_normed'  the memory m of the cross-attention skips PreNorm2's LayerNorm
    'patch_order'        a token's K index is (c p1 p2) in place of (p1 p2 c)
    'cross_swapped'      the cross-attention's projections change places: to_k sees x and makes the queries, to_q sees m and
                         makes the keys (q from m as far as the shapes allow: 1024 queries cannot come from 64 tokens)
    'outer_skip'         BasicModule('residual') adds its input, as BasicModule('basic') does
    'mean_folded'        sub_mean folded into head: head's zero padding sees sub_mean's INPUT, so the border taps miss the bias
    'qkv_order'          to_qkv's chunks taken as k | q | v
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BROKEN = ('scale_dim_head', 'gelu_erf', 'decoder_order', 'memory_not_normed', 'patch_order', 'cross_swapped', 'outer_skip',
          'mean_folded', 'qkv_order')
P = 8
DIM = 512
HEADS = 6
DIM_HEAD = 32
GOLDEN_CAP = 2048                          # two cases record 37 tensors each: the file stays about the size of hat.npz
GOLDEN_KEEP = 1024

# ---- the cases of tests/golden/transenet.npz (tools/make_transenet_golden.py runs the reference on them) ----
SEED = 17                                  # of synth.synth_transenet
SMALL = dict(n_feats=16, en_depth=2, de_depth=1)
FULL = dict(n_feats=64, en_depth=8, de_depth=1)      # the reference's
# name: (configuration, scale, batch, (H, W) of the LR input, taps checked, in the golden file); hr_patch_size = H * scale
CASES = {
    's4_32x32': (SMALL, 4, 1, (32, 32), True, True),      # N_low 16 (half an MFMA tile), N_high 256
    's4_32x16': (SMALL, 4, 1, (32, 16), True, True),      # N_low 8, N_high 128; an off-square W inferred by the rearrange
    's4_32x40': (SMALL, 4, 1, (32, 40), False, True),     # N_low 20, N_high 160: no multiple of 32, nor of a 128-key chunk
    's3_32x32': (SMALL, 3, 1, (32, 32), False, True),     # N_high 144; shuffle r = 3; 9 n_feats
    's2_32x32': (SMALL, 2, 1, (32, 32), False, True),     # N_high 64 = N_low * 4; one upsampler stage
    's8_32x32': (SMALL, 8, 1, (32, 32), False, False),    # restatement only: N_high 1024, eight key chunks; three stages
    'full_64x64': (FULL, 4, 1, (64, 64), False, True),    # the reference's shape: 64 / 1024 tokens, K = 1024
    'full_64x32_b2': (FULL, 4, 2, (64, 32), False, False),  # restatement only: N_low 32, N_high 512; batch stride
}
GOLDEN_CASES = [k for k, v in CASES.items() if v[5]]


def case_config(name):
    from fastdiffsr_amd.transenet.arch import TransENetConfig
    base, scale, _, hw, _, _ = CASES[name]
    return TransENetConfig(scale=scale, hr_patch_size=hw[0] * scale, **base)


def case_input(name, b, h, w):
    """[b, 3, h, w] in [0, 1): the input of a case, from the case's name."""
    return torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(zlib.crc32(name.encode())))


def recorded_taps(cfg):
    """Of arch.tap_names, the taps a case with taps records and the tests check: the convolutional front, each patch embedding,
    the first layer of every encoder and its end, every decoder's first layer, the tail."""
    from fastdiffsr_amd.transenet.arch import tap_names
    keep = []
    for t in tap_names(cfg):
        parts = t.split('.')
        if t.startswith(('encoder', 'decoder')) and len(parts) == 3 and parts[1] != '0':
            continue
        keep.append(t)
    return keep


def sample_index(key, numel, cap=GOLDEN_CAP, keep=GOLDEN_KEEP):
    """tests/golden/transenet.npz keeps a tensor of more than `cap` elements as a fixed sample of `keep` of its flat elements:
    the sorted flat indices of that sample, or None for a tensor kept whole."""
    if numel <= cap:
        return None
    return np.sort(np.random.default_rng(zlib.crc32(key.encode())).choice(numel, keep, replace=False))


def sampled(key, t):
    """The elements of tensor / array t that the golden file holds under `key`, flat."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    idx = sample_index(key, a.size)
    return a.reshape(-1) if idx is None else a.reshape(-1)[idx]


def _conv(t, wt, name, padding=1):
    """t is NCHW."""
    return F.conv2d(t, wt[name + '.weight'], wt[name + '.bias'], padding=padding)


def _linear(t, wt, name):
    return F.linear(t, wt[name + '.weight'], wt.get(name + '.bias'))


def _ln(t, wt, name):
    return F.layer_norm(t, (t.shape[-1],), wt[name + '.weight'], wt[name + '.bias'], 1e-5)


def _gelu(t, broken):
    if broken == 'gelu_erf':
        return F.gelu(t)
    return 0.5 * t * (1 + torch.tanh(np.sqrt(2 / np.pi) * (t + 0.044715 * t ** 3)))


def _heads(t):
    b, n, _ = t.shape
    return t.reshape(b, n, HEADS, DIM_HEAD).transpose(1, 2)          # 'b n (h d) -> b h n d'


def _attend(q, k, v, broken):
    scale = (DIM_HEAD if broken == 'scale_dim_head' else DIM) ** -0.5
    dots = (_heads(q) @ _heads(k).transpose(-2, -1)) * scale
    o = torch.softmax(dots, -1) @ _heads(v)
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[1], HEADS * DIM_HEAD)


def _self_attention(x, wt, p, broken):
    qkv = _linear(_ln(x, wt, p + '.fn.norm'), wt, p + '.fn.fn.to_qkv').chunk(3, -1)
    q, k, v = (qkv[1], qkv[0], qkv[2]) if broken == 'qkv_order' else qkv
    return x + _linear(_attend(q, k, v, broken), wt, p + '.fn.fn.to_out.0')


def _cross_attention(x, m, wt, p, broken):
    n = _ln(x, wt, p + '.fn.norm')
    nm = m if broken == 'memory_not_normed' else _ln(m, wt, p + '.fn.norm')
    tq, tk = ('to_k', 'to_q') if broken == 'cross_swapped' else ('to_q', 'to_k')
    q, k, v = _linear(n, wt, f'{p}.fn.fn.{tq}'), _linear(nm, wt, f'{p}.fn.fn.{tk}'), _linear(nm, wt, p + '.fn.fn.to_v')
    return x + _linear(_attend(q, k, v, broken), wt, p + '.fn.fn.to_out.0')


def _feed_forward(x, wt, p, broken):
    return x + _linear(_gelu(_linear(_ln(x, wt, p + '.fn.norm'), wt, p + '.fn.fn.net.0'), broken), wt, p + '.fn.fn.net.3')


def _patches(t, broken):
    """[B, C, H, W] -> [B, (h w), (p1 p2 c)]"""
    b, c, hh, ww = t.shape
    t = t.reshape(b, c, hh // P, P, ww // P, P)
    if broken == 'patch_order':
        return t.permute(0, 2, 4, 1, 3, 5).reshape(b, (hh // P) * (ww // P), c * P * P)
    return t.permute(0, 2, 4, 3, 5, 1).reshape(b, (hh // P) * (ww // P), P * P * c)


def _unpatches(t, h, w):
    """[B, (h w), (p1 p2 c)] -> [B, C, h 8, w 8]"""
    b = t.shape[0]
    return t.reshape(b, h, w, P, P, -1).permute(0, 5, 1, 3, 2, 4).reshape(b, -1, h * P, w * P)


def transenet_forward(weights, cfg, x, dtype=torch.float64, broken=None):
    assert broken is None or broken in BROKEN
    wt = {k: torch.as_tensor(v).to(device=x.device, dtype=dtype) for k, v in weights.items()}
    taps = {}
    x = x.to(dtype)
    b, _, h, w = x.shape
    assert h % P == 0 and w % P == 0
    hl, wl, hh, wh = h // P, w // P, h * cfg.scale // P, w * cfg.scale // P

    def tok_tap(name, t, hw):
        taps[name] = t.reshape(b, hw[0], hw[1], DIM).permute(0, 3, 1, 2).contiguous()

    t = _conv(x, wt, 'sub_mean', 0)
    if broken == 'mean_folded':
        # head(sub_mean(.)) as ONE convolution over the zero-padded input: the padding ring holds sub_mean(0) = its bias
        ring = wt['sub_mean.bias'].reshape(1, 3, 1, 1).expand(b, 3, h + 2, w + 2).clone()
        ring[:, :, 1:-1, 1:-1] = t
        f = _conv(ring, wt, 'head.0', 0)
    else:
        f = _conv(t, wt, 'head.0')
    taps['head'] = f
    low = []
    for s in (1, 2, 3):
        y = f
        for i in range(5):
            p = f'feat_extrat_stage{s}.body.{i}.body'
            y = _conv(F.relu(_conv(y, wt, p + '.0')), wt, p + '.2') + y
        if broken == 'outer_skip':
            y = y + f
        taps[f'stage{s}'] = y
        low.append(_conv(y, wt, f'stage{s}_conv1x1', 0))
        taps[f'stage{s}.1x1'] = low[-1]
    u = taps['stage3']
    for idx, r in cfg.upsample_convs():
        u = F.pixel_shuffle(_conv(u, wt, f'upsampler.{idx}'), r)
    taps['up'] = u
    hi = _conv(u, wt, 'up_conv1x1', 0)
    taps['up.1x1'] = hi

    toks = [_linear(_patches(low[i], broken), wt, f'patch_to_embedding_low{i + 1}') for i in range(3)]
    toks.append(_linear(_patches(hi, broken), wt, 'patch_to_embedding_high'))
    grids = [(hl, wl)] * 3 + [(hh, wh)]
    for i, name in enumerate(('embed.low1', 'embed.low2', 'embed.low3', 'embed.high')):
        tok_tap(name, toks[i], grids[i])
    for i, e in enumerate(('encoder_stage1', 'encoder_stage2', 'encoder_stage3', 'encoder_up')):
        y = toks[i]
        for j in range(cfg.en_depth):
            y = _self_attention(y, wt, f'{e}.layers.{j}.0', broken)
            tok_tap(f'{e}.{j}.attn', y, grids[i])
            y = _feed_forward(y, wt, f'{e}.layers.{j}.1', broken)
            tok_tap(f'{e}.{j}.ff', y, grids[i])
        tok_tap(e, y, grids[i])
        toks[i] = y
    y = toks[3]
    for d in ((1, 2, 3) if broken == 'decoder_order' else (3, 2, 1)):
        for j in range(cfg.de_depth):
            p = f'decoder{d}.layers.{j}'
            y = _self_attention(y, wt, p + '.0', broken)
            tok_tap(f'decoder{d}.{j}.self', y, grids[3])
            y = _cross_attention(y, toks[d - 1], wt, p + '.1', broken)
            tok_tap(f'decoder{d}.{j}.cross', y, grids[3])
            y = _feed_forward(y, wt, p + '.2', broken)
            tok_tap(f'decoder{d}.{j}.ff', y, grids[3])
    pm = _unpatches(_linear(y, wt, 'embedding_to_patch'), hh, wh)
    taps['embedding_to_patch'] = pm
    sp = _conv(pm, wt, 'span_conv1x1', 0)
    taps['span'] = sp
    taps['out'] = _conv(_conv(sp, wt, 'tail'), wt, 'add_mean', 0).contiguous()
    return taps


def save_img1(x):
    """[3, H, W] float tensor -> HWC uint8, the arithmetic of the reference's srutils.save_img1: times 255, clamp, truncate."""
    return (x * 255.0).clamp(0, 255).detach().cpu().numpy().transpose(1, 2, 0).astype('uint8')
