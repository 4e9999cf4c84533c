"""TransENet on the HIP engine (include/fdsr.h: fdsr_transenet_*): an nn.Module that takes the constructor arguments of the
reference's TransENet (MSI_SR_model/model/transenet.py) with the reference's defaults, owns its parameters under the
reference's names -- `generator_param.pkl` loads with load_state_dict -- and whose forward runs the device kernels.  Inference
only, exact fp32; there is no PyTorch fallback.  As in the reference, a module built for hr_patch_size computes images of LR
height hr_patch_size / scale only (the inverse patch rearrange is called with h = hr_patch_size // 8); the width is free."""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._engine_module import EngineModule
from ..swinir.model import to_u8  # noqa: F401  (save_img1 is the same function in transenet.py)
from .arch import MIN_NUM_PATCHES, PATCH, DIM, TransENetConfig, state_schema, tap_names


class TransENet(EngineModule):
    _family, _tap_names = 'transenet', staticmethod(tap_names)

    def __init__(self, n_feats=64, scale=4, n_basic_modules=10, n_colors=3, hr_patch_size=256, back_projection_iters=10, en_depth=8,
                 de_depth=1, conv=None):
        """n_basic_modules and back_projection_iters are unused by the reference too; conv must be its default_conv (or None)."""
        super().__init__()
        if conv is not None and getattr(conv, '__name__', '') != 'default_conv':
            raise NotImplementedError('TransENet on the HIP engine runs the reference\'s default_conv only')
        if n_colors != 3:
            raise NotImplementedError('TransENet on the HIP engine does not run n_colors %r (only 3)' % (n_colors,))
        if scale not in (2, 3, 4, 8):
            raise NotImplementedError('TransENet on the HIP engine does not run scale %r (only 2, 3, 4, 8)' % (scale,))
        image_size = hr_patch_size // scale
        # the reference's two constructor assertions
        if hr_patch_size % scale or image_size % PATCH:
            raise ValueError('Image dimensions must be divisible by the patch size: hr_patch_size %r / scale %r is no multiple of 8'
                             % (hr_patch_size, scale))
        if (image_size // PATCH) ** 2 <= MIN_NUM_PATCHES:
            raise ValueError('your number of patches (%d) is way too small for attention to be effective: the LR side '
                             'hr_patch_size / scale must be at least 32' % ((image_size // PATCH) ** 2))
        self.cfg = TransENetConfig(n_feats, scale, n_colors, hr_patch_size, en_depth, de_depth)
        self.scale, self.hr_patch_size, self.patch_size = scale, hr_patch_size, PATCH
        self.schema = state_schema(self.cfg)
        # dotted names cannot be registered on an nn.Module: the tensors live under p<i> and state_dict / load_state_dict speak
        # the reference's keys
        self._names = list(self.schema)
        for i, shape in enumerate(self.schema.values()):
            self.register_parameter('p%d' % i, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._init_engine()     # refuses what the kernels do not cover (n_feats, depths) with the library's message

    def load_reference_state_dict(self, state_dict, strict=False):
        """The reference's own TransENet.load_state_dict: a known key is copied; a shape mismatch is an error except under 'tail'
        (a checkpoint of another scale keeps its body); an unknown key counts only with strict, and not under 'tail'; with strict
        every key of the model must be there."""
        own = self.state_dict()
        for name, param in state_dict.items():
            if name in own:
                if tuple(param.shape) != tuple(own[name].shape):
                    if 'tail' in name:
                        continue
                    raise RuntimeError('While copying the parameter named {}, whose dimensions in the model are {} and whose '
                                       'dimensions in the checkpoint are {}.'.format(name, tuple(own[name].shape), tuple(param.shape)))
                with torch.no_grad():
                    own[name].copy_(param)     # bumps _version: the next forward uploads it
            elif strict and 'tail' not in name:
                raise KeyError('unexpected key "{}" in state_dict'.format(name))
        if strict:
            missing = set(own) - set(state_dict)
            if missing:
                raise KeyError('missing keys in state_dict: "{}"'.format(sorted(missing)))

    def named_reference_parameters(self):
        return [(k, getattr(self, 'p%d' % i)) for i, k in enumerate(self._names)]

    # ---- the engine ----
    def _fill_config(self):
        cfg = self.cfg
        c = _lib.FdsrTransenetConfig()
        c.n_feats, c.scale, c.n_colors, c.en_depth, c.de_depth = cfg.n_feats, cfg.scale, cfg.n_colors, cfg.en_depth, cfg.de_depth
        return c

    def _check(self, x):
        if not (torch.is_tensor(x) and x.dim() == 4 and x.shape[1] == 3):
            raise ValueError('TransENet takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        h, w = int(x.shape[2]), int(x.shape[3])
        if h % PATCH or w % PATCH:
            raise ValueError('TransENet takes sides that are multiples of the patch size 8, not %dx%d' % (h, w))
        if h * self.scale != self.hr_patch_size:
            raise ValueError("TransENet built with hr_patch_size %d at scale %d computes inputs of height %d only, not %d: the "
                             "reference's rearrange(feat_ups, 'b (h w) (p1 p2 c) -> b c (h p1) (w p2)', h=self.hr_patch_size // p) "
                             "fixes the HR height (the width is inferred)" % (self.hr_patch_size, self.scale,
                                                                              self.hr_patch_size // self.scale, h))
        if not x.is_cuda:
            raise ValueError('TransENet takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        return x.float().contiguous()

    def output_shape(self, b, h, w):
        """H = hr_patch_size / scale: see _check."""
        return (b, 3, h * self.scale, w * self.scale)

    def _debug_capacity(self, b, h, w):
        # the largest: n_feats channels at HR; tokens are DIM per 64 pixels
        return b * h * w * self.scale ** 2 * max(self.cfg.n_feats, DIM // (PATCH * PATCH))


def load_synthetic(model, seed=0):
    """Fill a TransENet with synth.synth_transenet's weights (tests, timing, smoke runs)."""
    from ..synth import synth_transenet
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth_transenet(model.cfg, seed).items()}
    model.load_state_dict(sd, strict=True)
    return model
