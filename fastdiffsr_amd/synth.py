"""Portable synthetic ("random-init") weights for the FastDiffSR UNet.

Every tensor of the checkpoint schema (arch.param_schema) is defined by a
closed-form, platform-stable generator seeded from its own key, so the same
arrays are produced in the build container (where they are loaded into the
imported reference to make tests/golden/*) and on the GPU box (where they are
loaded into the HIP engine and the oracle).  No 95 MB checkpoint is committed;
tests pin the generator through a SHA-256 of the concatenated bytes.

Scales: conv/linear weights ~ N(0, 0.7^2 * 2/fan_in) keep activations O(1)
through the 29-layer stack; GroupNorm gamma = 1 + 0.1 N, every bias / beta =
0.05 N, so bias, affine and FiLM-shift arithmetic is exercised (PyTorch's
default init has gamma=1, beta=0).  SURVEY.md section 7 stage 0 / App. E.
"""
import hashlib
from collections import OrderedDict

import numpy as np

from .arch import UNetConfig, param_schema


def _rng(key: str, seed: int) -> np.random.Generator:
    h = hashlib.sha256(f'{seed}:{key}'.encode()).digest()
    return np.random.Generator(np.random.PCG64(int.from_bytes(h[:8], 'little')))


def synth_tensor(key: str, shape, seed: int = 0) -> np.ndarray:
    if key.endswith('inv_freq'):     # TimeEmbedding buffer (ddpm_modules/unet.py:22-27), formed in fp32 like torch does
        import torch
        dim = 2 * shape[0]
        return torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * (-np.log(10000) / dim)).numpy()
    g = _rng(key, seed)
    x = g.standard_normal(size=shape, dtype=np.float64)
    if key.endswith('.bias'):
        x *= 0.05
    elif len(shape) == 1:          # GroupNorm gamma (incl. attn.norm)
        x = 1.0 + 0.1 * x
    else:
        fan_in = int(np.prod(shape[1:]))
        x *= 0.7 * np.sqrt(2.0 / fan_in)
    return x.astype(np.float32)


def synth_state_dict(cfg: UNetConfig, seed: int = 0, prefix: str = '') -> "OrderedDict[str, np.ndarray]":
    """All UNet tensors (numpy fp32), keys optionally prefixed (e.g. 'denoise_fn.')."""
    out = OrderedDict()
    for k, shp in param_schema(cfg).items():
        out[prefix + k] = synth_tensor(k, shp, seed)
    return out


def state_dict_sha256(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v, dtype=np.float32).tobytes())
    return h.hexdigest()


def synth_inputs(batch: int, height: int, width: int, steps: int = 20,
                 cond_seed: int = 1234, noise_seed: int = 4321):
    """Synthetic conditioning image U(-1,1) and noise N(0,1).

    Returned as torch CPU tensors: cond [B,3,H,W], noise [steps,B,3,H,W];
    noise[0] is x_T, noise[k] feeds the step t = steps-k."""
    import torch
    g = torch.Generator().manual_seed(cond_seed)
    cond = torch.rand(batch, 3, height, width, generator=g) * 2.0 - 1.0
    g = torch.Generator().manual_seed(noise_seed)
    noise = torch.randn(steps, batch, 3, height, width, generator=g)
    return cond, noise


def synth_alexnet_features(seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """A stand-in for torchvision's ImageNet AlexNet `features` (the LPIPS backbone; no real copy is committed): the ten
    torchvision-keyed tensors, float32, drawn in key order from numpy.random.default_rng(seed) -- weights He-normal
    (std sqrt(2 / fan_in)), biases N(0, 0.05^2).  tests/golden/lpips_alex.npz records a per-tensor checksum of them."""
    from .metrics import LPIPS_BACKBONE
    g = np.random.default_rng(seed)
    out = OrderedDict()
    for k, shape in LPIPS_BACKBONE.items():
        if k.endswith('.bias'):
            x = g.normal(0.0, 0.05, size=shape)
        else:
            x = g.normal(0.0, np.sqrt(2.0 / int(np.prod(shape[1:]))), size=shape)
        out[k] = x.astype(np.float32)
    return out


def synth_inception_fid(seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """A stand-in for pytorch_fid's FID Inception weights (pt_inception-2015-12-05-6726825d.pth; no real copy is committed):
    the 470 tensors of metrics.FID_TENSORS, float32, drawn in key order from numpy.random.default_rng(seed) -- conv weights
    He-normal (std sqrt(2 / fan_in)), BN gamma N(1, 0.05^2), beta N(0, 0.05^2), running mean 0 and var 1 -- so that every
    block's activations stay O(1) (tests/test_fid_host.py checks it)."""
    from .metrics import FID_TENSORS
    g = np.random.default_rng(seed)
    out = OrderedDict()
    for k, shape in FID_TENSORS.items():
        if k.endswith('.conv.weight'):
            x = g.normal(0.0, np.sqrt(2.0 / int(np.prod(shape[1:]))), size=shape)
        elif k.endswith('.bn.weight'):
            x = g.normal(1.0, 0.05, size=shape)
        elif k.endswith('.bn.bias'):
            x = g.normal(0.0, 0.05, size=shape)
        elif k.endswith('.bn.running_mean'):
            x = np.zeros(shape)
        else:
            x = np.ones(shape)
        out[k] = x.astype(np.float32)
    return out


def synth_swinir(cfg, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights for SwinIR, keyed and ordered as swinir.arch.param_schema(cfg), every tensor from its own key.  Not
    the reference's init: trunc_normal_(std=.02) gives nearly flat attention, under which a wrong mask, bias index or roll
    disappears.  Here the q and k rows of qkv are N(0, 1.5 / C), so the logits q k^T / sqrt(head_dim) have a spread of about
    1.5; the bias table is N(0, 1); every LayerNorm has weight 1 + 0.2 N and bias 0.1 N; proj and fc2 are damped (variance
    0.1 / fan_in and 0.6 / fan_in: fc2 strong enough that the tanh form of GELU shows at the output) and the RSTB convolutions N(0, 0.5 / fan_in), so the residual stream stays O(1) through
    all 36 blocks; the other weights are N(0, g / fan_in) with g between 1 and 4, biases 0.05 N (qkv 0.1 N)."""
    from .swinir.arch import param_schema as swin_schema
    c = cfg.embed_dim
    out = OrderedDict()
    for k, shape in swin_schema(cfg).items():
        x = _rng('swinir:' + k, seed).standard_normal(size=shape, dtype=np.float64)
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        norm = '.norm' in k or k.startswith('norm.')
        if k.endswith('relative_position_bias_table'):
            pass
        elif norm and k.endswith('.weight'):
            x = 1.0 + 0.2 * x
        elif norm:
            x *= 0.1
        elif k.endswith('.bias'):
            x *= 0.1 if '.qkv.' in k else 0.05
        elif '.qkv.' in k:
            x *= np.sqrt(np.r_[np.full(2 * c, 1.5), np.ones(c)] / fan_in)[:, None]
        else:
            gain = {'proj': 0.1, 'fc1': 2.0, 'fc2': 0.6, 'conv': 0.5, 'conv_first': 4.0, 'conv_after_body': 1.0, '0': 2.0, '2': 2.0,
                    '4': 2.0, 'conv_last': 1.0}[k.split('.')[-2]]
            x *= np.sqrt(gain / fan_in)
        out[k] = x.astype(np.float32)
    return out


def synth_hat(cfg, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights for HAT, keyed and ordered as hat.arch.param_schema(cfg) (one entry for the shared upsampling
    convolution), every tensor from its own key, in the spirit of synth_swinir: the q and k rows of both qkv kinds are
    N(0, 1.5 / C) (a logit spread of about 1.5 in the window attention and in the overlapping cross-attention), both bias tables
    N(0, 1), LayerNorms 1 + 0.2 N / 0.1 N, proj damped (variance 0.1 / fan_in) and the RHAG convolutions N(0, 0.2 / fan_in) so
    that the residual stream stays O(1) through every HAB and OCAB (below 40 at every tap of the full configuration).  fc1 and
    fc2 are strong (4 / fan_in and 2.5 / fan_in: pre-activations of about 2, where the erf and tanh forms of GELU differ most,
    so that the tanh form shows at the output by more than 100 times the fp32 noise).  The CAB is made to matter although
    conv_scale is 0.01: its second convolution is N(0, 8 / fan_in) with a bias of 0.5 N, so the pooled channel means are not
    all near zero, and the two 1x1 layers of the gate have gains 16 and 8, so the gate's logits spread over a few units (a
    sigmoid that is dropped, or a pool over the wrong area, moves the gate visibly)."""
    from .hat.arch import param_schema as hat_schema
    c = cfg.embed_dim
    out = OrderedDict()
    for k, shape in hat_schema(cfg).items():
        x = _rng('hat:' + k, seed).standard_normal(size=shape, dtype=np.float64)
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        norm = '.norm' in k or k.startswith('norm.')
        if k.endswith('relative_position_bias_table'):
            pass
        elif norm and k.endswith('.weight'):
            x = 1.0 + 0.2 * x
        elif norm:
            x *= 0.1
        elif k.endswith('.bias'):
            x *= 0.5 if '.cab.2.' in k else 0.1 if ('.qkv.' in k or '.attention.' in k) else 0.05
        elif '.qkv.' in k:
            x *= np.sqrt(np.r_[np.full(2 * c, 1.5), np.ones(c)] / fan_in)[:, None]
        else:
            if '.cab.' in k:
                gain = {'0': 2.0, '2': 8.0, '1': 16.0, '3': 8.0}[k.split('.')[-2]]
            else:
                gain = {'proj': 0.1, 'fc1': 4.0, 'fc2': 2.5, 'conv': 0.2, 'conv_first': 4.0, 'conv_after_body': 1.0, '0': 2.0,
                        'conv_last': 1.0}[k.split('.')[-2]]
            x *= np.sqrt(gain / fan_in)
        out[k] = x.astype(np.float32)
    return out


def synth_transenet(cfg, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights for TransENet, keyed and ordered as transenet.arch.state_schema(cfg), every tensor from its own key,
    in the spirit of synth_hat.  The reference scales its logits by dim ** -0.5 = 512^-0.5 although a head has 32 dimensions:
    q . k over 32 terms of variance s^2 each has a spread of sqrt(32) s^2, so the rows of to_qkv that make q and k, and to_q and
    to_k, are N(0, 6 / 512) (s^2 = 6 on a LayerNorm's output): a logit spread of sqrt(32) 6 / sqrt(512) = 1.5 in every
    attention, self and cross, at 8 keys and at 1024.  The v rows are N(0, 1 / 512).  LayerNorms are 1 + 0.2 N / 0.1 N.  to_out is
    N(0, 0.5 / fan_in); net.0 and net.3 are N(0, 4 / fan_in) and N(0, 2 / fan_in) (pre-activations of about 2, where the erf and
    tanh forms of GELU differ most).  sub_mean and add_mean are perturbed off what the reference initialises them to (the identity
    and -/+ the mean): weight I + 0.15 N, bias -/+ mean + 0.05 N, so that a folded or skipped MeanShift shows.  The ResBlocks'
    first convolution is N(0, 2 / fan_in), the second N(0, 0.5 / fan_in); the other convolutions and Linears N(0, g / fan_in), g
    between 1 and 4; biases 0.05 N."""
    from .transenet.arch import RGB_MEAN as TE_MEAN, INNER, state_schema as te_schema
    out = OrderedDict()
    for k, shape in te_schema(cfg).items():
        x = _rng('transenet:' + k, seed).standard_normal(size=shape, dtype=np.float64)
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        mod = k.rsplit('.', 1)[0]
        if mod in ('sub_mean', 'add_mean'):
            sign = -1.0 if mod == 'sub_mean' else 1.0
            x = (np.eye(3).reshape(3, 3, 1, 1) + 0.15 * x) if k.endswith('.weight') else (sign * np.asarray(TE_MEAN) + 0.05 * x)
        elif mod.endswith('.norm'):
            x = 1.0 + 0.2 * x if k.endswith('.weight') else 0.1 * x
        elif k.endswith('.bias'):
            x *= 0.05
        elif mod.endswith('.to_qkv'):
            x *= np.sqrt(np.r_[np.full(2 * INNER, 6.0), np.ones(INNER)] / fan_in)[:, None]
        else:
            parts = mod.split('.')
            if mod.startswith('feat_extrat_stage'):
                gain = 2.0 if parts[-1] == '0' else 0.5
            elif mod.startswith('upsampler.'):
                gain = 2.0
            elif parts[-1] in ('to_q', 'to_k'):
                gain = 6.0
            else:
                gain = {'to_out.0': 0.5, 'net.0': 4.0, 'net.3': 2.0, 'head.0': 4.0}.get('.'.join(parts[-2:]), 1.0)
            x *= np.sqrt(gain / fan_in)
        out[k] = x.astype(np.float32)
    return out


HSENET_QK_GAIN = 2.0       # synth_hsenet's default (load_synthetic, the timing tool): softmax rows of the ten-module network neither flat nor one-hot


def synth_hsenet(cfg, seed: int = 0, qk_gain: float = HSENET_QK_GAIN) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights for HSENet, keyed and ordered as hsenet.arch.state_schema(cfg), every tensor from its own key.  The
    3x3 convolutions are N(0, 1 / fan_in) (each is followed by a ReLU, and every module adds to a residual stream that grows
    through the network), head.0 N(0, 4 / fan_in), g N(0, 1 / fan_in), AB.1 N(0, 4 / fan_in) (gate logits of a few units);
    biases 0.05 N.  The reference initialises every W of a non-local block to ZERO, which makes the block the identity; here W
    is N(0, 1 / fan_in).  The logits theta(x)^T phi(x) are unscaled: under plain fan-in weights the softmax over hundreds of
    pixels is flat and the attention a mean, so theta and phi are N(0, 1 / fan_in) times qk_gain (the logits grow with its
    square); tests fix a gain per configuration from a probe of the fp64 restatement (tests/hsenet_restatement.py).  sub_mean
    and add_mean are the reference's constants: the identity and -/+ the UCMerced mean (std 1)."""
    from .hsenet.arch import RGB_MEAN as HS_MEAN, state_schema as hs_schema
    out = OrderedDict()
    for k, shape in hs_schema(cfg).items():
        x = _rng('hsenet:' + k, seed).standard_normal(size=shape, dtype=np.float64)
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        mod = k.rsplit('.', 1)[0]
        if mod in ('sub_mean', 'add_mean'):
            sign = -1.0 if mod == 'sub_mean' else 1.0
            x = np.eye(3).reshape(3, 3, 1, 1) if k.endswith('.weight') else sign * np.asarray(HS_MEAN)
        elif k.endswith('.bias'):
            x *= 0.05
        else:
            last = mod.split('.')[-1]
            gain = 4.0 if mod == 'head.0' or mod.endswith('.AB.1') else 1.0
            x *= np.sqrt(gain / fan_in) * (qk_gain if last in ('theta', 'phi') else 1.0)
        out[k] = x.astype(np.float32)
    return out


def synth_nafnet(seed: int = 0, width: int = 16, enc_blk_nums=(2, 1, 1, 1), middle_blk_num: int = 1, dec_blk_nums=(1, 1, 1, 1),
                 img_channel: int = 3) -> "OrderedDict[str, np.ndarray]":
    """Synthetic weights for EDiffSR's ConditionalNAFNet, keyed and ordered as ediffsr.arch.param_schema.  The reference
    initialises every beta / gamma to ZERO, which makes every NAFBlock the identity; here beta, gamma ~ 0.3 N(0,1), biases
    0.05 N(0,1), LayerNorm g = 1 + 0.1 N(0,1), conv / linear weights N(0, 1/(3 fan_in)) (the variance of torch's default
    kaiming_uniform(a=sqrt(5)) init) -- every tensor from its own key."""
    from .ediffsr.arch import NAFNetConfig, param_schema as naf_schema
    cfg = NAFNetConfig(img_channel, width, middle_blk_num, list(enc_blk_nums), list(dec_blk_nums))
    out = OrderedDict()
    for k, shape in naf_schema(cfg).items():
        x = _rng('nafnet:' + k, seed).standard_normal(size=shape, dtype=np.float64)
        if k.endswith(('.beta', '.gamma')):
            x *= 0.3
        elif k.endswith('.bias'):
            x *= 0.05
        elif k.endswith('.g'):
            x = 1.0 + 0.1 * x
        else:
            x *= np.sqrt(1.0 / (3 * int(np.prod(shape[1:]))))
        out[k] = x.astype(np.float32)
    return out
