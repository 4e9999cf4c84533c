"""HSENet restated in plain torch from the architecture (not a test module; tests import it): the network that
fastdiffsr_amd.hsenet runs on the device, written functionally over a dict of weights under the reference's state_dict names,
runnable in fp32 and fp64 on the CPU or, for timing, on a GPU.

    taps = hsenet_forward(weights, cfg, x, dtype=torch.float64)

returns every named tap of hsenet.arch.tap_names(cfg) as NCHW and 'out'.  `stats`, a list, receives one record per attention
call: (Nq, Nk, median row maximum of the softmax, largest row maximum, largest |logit|).  `broken` switches one piece to a
plausible wrong form, so that a test can show that its tolerance would catch it:
    'softmax_scaled'        the logits are scaled by inter_channels ** -0.5, as a transformer's are
    'softmax_over_queries'  the softmax runs over the query axis
    'cross_swapped'         theta and phi change places in the AdjustedNonLocalBlock
    'cross_residual_x1'     the AdjustedNonLocalBlock adds x1 (the upsampled half-scale branch) in place of x0
    'g_from_query'          the AdjustedNonLocalBlock takes its values g from x1, the queries' side
    'align_corners'         the upsampling back to the base scale uses align_corners=True
    'down_corner_pixel'     the half scale takes pixel (2i, 2j) in place of the mean of four
    'gate_skips_1x1'        sigmoid of the non-local block's output, without AB.1
    'ssem_no_relu'          the SSEM's BasicBlocks without their ReLU (they pass no act, but the default is ReLU)
    'no_outer_skip'         the body's output without + head's output
    'mean_folded'           sub_mean folded into head: head's zero padding sees sub_mean's INPUT, so the border taps miss the bias
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BROKEN = ('softmax_scaled', 'softmax_over_queries', 'cross_swapped', 'cross_residual_x1', 'g_from_query', 'align_corners',
          'down_corner_pixel', 'gate_skips_1x1', 'ssem_no_relu', 'no_outer_skip', 'mean_folded')
GOLDEN_CAP = 2048
GOLDEN_KEEP = 1024

# ---- the cases of tests/golden/hsenet.npz (tools/make_hsenet_golden.py runs the reference on them) ----
SEED = 23                                  # of synth.synth_hsenet
SMALL = dict(n_feats=16, n_basic_modules=2)
MID = dict(n_feats=32, n_basic_modules=2)
WIDE = dict(n_feats=64, n_basic_modules=2)
FULL = dict(n_feats=64, n_basic_modules=10)          # the reference's
# theta / phi gains of synth_hsenet per configuration, fixed from a probe of the fp64 restatement so that the softmax is neither
# flat nor one-hot (test_hsenet_host.py checks the conditions); activations grow through the modules, so FULL needs less
GAIN_SMALL, GAIN_MID, GAIN_FULL, GAIN_SHARP = 8.0, 6.0, 1.5, 10.0
# name: (configuration, qk_gain, scale, batch, (H, W) of the LR input, taps checked, in the golden file)
CASES = {
    's4_8x8': (SMALL, GAIN_SMALL, 4, 1, (8, 8), True, True),          # N 64; 16 half-scale keys, half an MFMA tile
    's4_9x7': (SMALL, GAIN_SMALL, 4, 1, (9, 7), True, True),          # N 63, half scale 4 x 3: both sides odd, a partial query block
    's4_12x20': (SMALL, GAIN_SMALL, 4, 1, (12, 20), False, True),     # N 240: two 128-key chunks, the last partial; off-square
    's3_13x16_b2': (SMALL, GAIN_SMALL, 3, 2, (13, 16), False, True),  # PixelShuffle(3), batch stride, one odd side
    's2_8x8': (SMALL, GAIN_SMALL, 2, 1, (8, 8), False, True),         # one upsampler stage
    's8_8x8': (SMALL, GAIN_SMALL, 8, 1, (8, 8), False, False),        # restatement only: three upsampler stages
    'm4_16x16': (MID, GAIN_MID, 4, 1, (16, 16), False, True),         # d = 16 padded to 32
    'sharp_16x16': (WIDE, GAIN_SHARP, 4, 1, (16, 16), False, False),  # restatement only: logits past 100, the max subtraction
    'full_32x32': (FULL, GAIN_FULL, 4, 1, (32, 32), False, True),     # N 1024 in eight chunks, 256 half-scale keys, ten modules
    'full_64x64': (FULL, GAIN_FULL, 4, 1, (64, 64), False, True),     # the reference's shape; N 4096
    'full_24x40_b2': (FULL, GAIN_FULL, 4, 2, (24, 40), False, False),  # restatement only: batch stride at d = 32, N 960
}
GOLDEN_CASES = [k for k, v in CASES.items() if v[6]]


def case_config(name):
    from fastdiffsr_amd.hsenet.arch import HSENetConfig
    base, _, scale, _, _, _, _ = CASES[name]
    return HSENetConfig(scale=scale, **base)


def case_weights(name):
    from fastdiffsr_amd.synth import synth_hsenet
    return synth_hsenet(case_config(name), SEED, CASES[name][1])


def case_input(name, b, h, w):
    """[b, 3, h, w] in [0, 1): the input of a case, from the case's name."""
    return torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(zlib.crc32(name.encode())))


def recorded_taps(cfg):
    """Of arch.tap_names, the taps a case with taps records and the tests check: everything of the first module, every later
    module's output, and the frame (head, body, up)."""
    from fastdiffsr_amd.hsenet.arch import tap_names
    return [t for t in tap_names(cfg) if '.' not in t or t.startswith('m0.')]


def sample_index(key, numel, cap=GOLDEN_CAP, keep=GOLDEN_KEEP):
    """tests/golden/hsenet.npz keeps a tensor of more than `cap` elements as a fixed sample of `keep` of its flat elements:
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
    return F.conv2d(t, wt[name + '.weight'], wt[name + '.bias'], padding=padding)


def down_half(t):
    """F.interpolate(t, scale_factor=0.5, mode='bilinear') (align_corners=False): the mean of pixels (2i, 2i + 1) x (2j, 2j + 1);
    an odd last row or column is dropped."""
    h, w = t.shape[2] // 2, t.shape[3] // 2
    t = t[:, :, :2 * h, :2 * w]
    return 0.25 * (t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2] + t[:, :, 1::2, 0::2] + t[:, :, 1::2, 1::2])


def up_to(t, size, align_corners=False):
    """F.interpolate(t, size=size, mode='bilinear'): source coordinate max(0, (o + 0.5) in / out - 0.5), neighbour clamped."""
    def axis(n_in, n_out):
        o = torch.arange(n_out, dtype=t.dtype, device=t.device)
        if align_corners:
            s = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else o * 0
        else:
            s = ((o + 0.5) * (n_in / n_out) - 0.5).clamp(min=0)
        i0 = s.floor().long().clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        return i0, i1, s - i0.to(t.dtype)
    y0, y1, ly = axis(t.shape[2], size[0])
    x0, x1, lx = axis(t.shape[3], size[1])
    ly = ly.reshape(1, 1, -1, 1)
    rows = t[:, :, y0] * (1 - ly) + t[:, :, y1] * ly
    return rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx


def _nonlocal(x0, x1, wt, p, broken, stats, cross):
    """W(softmax(theta(x1)^T phi(x0)) g(x0)) + x0; the self form has x1 = x0."""
    b, _, h, w = x1.shape
    tq, tk = ('phi', 'theta') if cross and broken == 'cross_swapped' else ('theta', 'phi')
    q = _conv(x1, wt, f'{p}.{tq}', 0).flatten(2).transpose(1, 2)                 # [B, Nq, d]
    k = _conv(x0, wt, f'{p}.{tk}', 0).flatten(2)                                   # [B, d, Nk]
    gsrc = x1 if cross and broken == 'g_from_query' else x0
    v = _conv(gsrc, wt, p + '.g', 0).flatten(2).transpose(1, 2)                   # [B, Nk, d]
    f = q @ k
    if broken == 'softmax_scaled':
        f = f * q.shape[-1] ** -0.5
    pr = torch.softmax(f, -2 if broken == 'softmax_over_queries' else -1)
    if stats is not None:
        rm = pr.max(-1).values
        stats.append((f.shape[1], f.shape[2], float(rm.median()), float(rm.max()), float(f.abs().max())))
    y = (pr @ v).transpose(1, 2).reshape(b, -1, h, w)
    return _conv(y, wt, p + '.W', 0) + (x1 if cross and broken == 'cross_residual_x1' else x0)


def _ssem(x, wt, p, broken, stats, taps, tp):
    act = (lambda t: t) if broken == 'ssem_no_relu' else F.relu
    hh = act(_conv(x, wt, p + '.head.0.0'))
    mb = act(_conv(act(_conv(hh, wt, p + '.MB.0.0')), wt, p + '.MB.1.0'))
    z = _nonlocal(hh, hh, wt, p + '.AB.0', broken, stats, False)
    taps[tp + '.nl'] = z
    gate = mb * torch.sigmoid(z if broken == 'gate_skips_1x1' else _conv(z, wt, p + '.AB.1', 0))
    taps[tp + '.gate'] = gate
    out = x + act(_conv(gate, wt, p + '.tail.0.0'))
    taps[tp] = out
    return out


def hsenet_forward(weights, cfg, x, dtype=torch.float64, broken=None, stats=None):
    assert broken is None or broken in BROKEN
    wt = {k: torch.as_tensor(v).to(device=x.device, dtype=dtype) for k, v in weights.items()}
    taps = {}
    x = x.to(dtype)
    b, _, h, w = x.shape
    t = _conv(x, wt, 'sub_mean', 0)
    if broken == 'mean_folded':
        # head(sub_mean(.)) as ONE convolution over the zero-padded input: the padding ring holds sub_mean(0) = its bias
        ring = wt['sub_mean.bias'].reshape(1, 3, 1, 1).expand(b, 3, h + 2, w + 2).clone()
        ring[:, :, 1:-1, 1:-1] = t
        f = _conv(ring, wt, 'head.0', 0)
    else:
        f = _conv(t, wt, 'head.0')
    taps['head'] = f
    y = f
    for i in range(cfg.n_basic_modules):
        p, tp = f'body_modulist.{i}', f'm{i}'
        s = F.relu(_conv(F.relu(_conv(y, wt, p + '.head.0.0')), wt, p + '.head.1.0'))
        taps[tp + '.head'] = s
        hp = p + '.body.0'
        xb = _ssem(s, wt, hp + '.base_scale.0', broken, stats, taps, tp + '.base')
        d = s[:, :, 0:2 * (h // 2):2, 0:2 * (w // 2):2] if broken == 'down_corner_pixel' else down_half(s)
        taps[tp + '.down.in'] = d
        xd = _ssem(d, wt, hp + '.down_scale.0', broken, stats, taps, tp + '.down')
        xu = up_to(xd, (h, w), align_corners=broken == 'align_corners')
        taps[tp + '.up'] = xu
        nl = _nonlocal(xb, xu, wt, hp + '.NonLocal_base', broken, stats, True)
        taps[tp + '.cross'] = nl
        hs = s + F.relu(_conv(nl, wt, hp + '.tail.0.0'))
        taps[tp + '.hsem'] = hs
        y = y + F.relu(_conv(F.relu(_conv(hs, wt, p + '.tail.0.0')), wt, p + '.tail.1.0'))
        taps[tp] = y
    u = y if broken == 'no_outer_skip' else y + f
    taps['body'] = u
    for idx, r in cfg.upsample_convs():
        u = F.pixel_shuffle(_conv(u, wt, f'tail.0.{idx}'), r)
    taps['up'] = u
    taps['out'] = _conv(_conv(u, wt, 'tail.1'), wt, 'add_mean', 0).contiguous()
    return taps
