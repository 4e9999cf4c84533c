"""HSENet on the HIP engine (include/fdsr.h: fdsr_hsenet_*): an nn.Module that takes the constructor arguments of the
reference's HSENET (MSI_SR_model/model/hsenet.py) with the reference's defaults, owns its parameters under the reference's
names -- `generator_param.pkl` loads with load_state_dict -- and whose forward runs the device kernels.  Inference only, exact
fp32; there is no PyTorch fallback.  Any [B, 3, H, W] with H, W >= 2 is computed: below that the reference's own half-scale
branch has no pixel."""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._engine_module import EngineModule
from ..swinir.model import to_u8  # noqa: F401  (save_img1 is the same function in hsenet.py)
from .arch import HSENetConfig, state_schema, tap_names


class HSENet(EngineModule):
    _family, _tap_names = 'hsenet', staticmethod(tap_names)

    def __init__(self, n_feats=64, scale=3, n_basic_modules=10, n_colors=3, conv=None):
        """conv must be the reference's default_conv (or None)."""
        super().__init__()
        if conv is not None and getattr(conv, '__name__', '') != 'default_conv':
            raise NotImplementedError('HSENet on the HIP engine runs the reference\'s default_conv only')
        if n_colors != 3:
            raise NotImplementedError('HSENet on the HIP engine does not run n_colors %r (only 3)' % (n_colors,))
        if scale not in (2, 3, 4, 8):
            raise NotImplementedError('HSENet on the HIP engine does not run scale %r (only 2, 3, 4, 8)' % (scale,))
        self.cfg = HSENetConfig(n_feats, scale, n_colors, n_basic_modules)
        self.scale = scale
        self.schema = state_schema(self.cfg)
        # dotted names cannot be registered on an nn.Module: the tensors live under p<i> and state_dict / load_state_dict speak
        # the reference's keys
        self._names = list(self.schema)
        for i, shape in enumerate(self.schema.values()):
            self.register_parameter('p%d' % i, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._init_engine()     # refuses what the kernels do not cover (n_feats, n_basic_modules) with the library's message

    def load_reference_state_dict(self, state_dict, strict=False):
        """The reference's own HSENET.load_state_dict: a known key is copied; a shape mismatch is an error except under 'tail'
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
        c = _lib.FdsrHsenetConfig()
        c.n_feats, c.scale, c.n_colors, c.n_basic_modules = cfg.n_feats, cfg.scale, cfg.n_colors, cfg.n_basic_modules
        return c

    def _check(self, x):
        if not (torch.is_tensor(x) and x.dim() == 4 and x.shape[1] == 3):
            raise ValueError('HSENet takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        h, w = int(x.shape[2]), int(x.shape[3])
        if h < 2 or w < 2:
            raise ValueError('HSENet takes sides of at least 2, not %dx%d: the half-scale branch of the reference\'s HSEM '
                             '(F.interpolate(x, scale_factor=0.5)) has no pixel below that' % (h, w))
        if not x.is_cuda:
            raise ValueError('HSENet takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        return x.float().contiguous()

    def output_shape(self, b, h, w):
        return (b, 3, h * self.scale, w * self.scale)

    def _debug_capacity(self, b, h, w):
        # the largest: n_feats channels at HR
        return b * h * w * self.scale ** 2 * self.cfg.n_feats


def load_synthetic(model, seed=0, qk_gain=None):
    """Fill an HSENet with synth.synth_hsenet's weights (tests, timing, smoke runs)."""
    from ..synth import HSENET_QK_GAIN, synth_hsenet
    sd = {k: torch.from_numpy(np.ascontiguousarray(v))
          for k, v in synth_hsenet(model.cfg, seed, HSENET_QK_GAIN if qk_gain is None else qk_gain).items()}
    model.load_state_dict(sd, strict=True)
    return model
