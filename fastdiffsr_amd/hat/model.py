"""HAT on the HIP engine (include/fdsr.h: fdsr_hat_*): an nn.Module that takes the constructor arguments of the reference's
GeneratorResNet (MSI_SR_model/model/hat.py) with the reference's defaults, owns its parameters and buffers under the
reference's names -- `generator_param.pkl` loads with load_state_dict(strict=True) -- and whose forward runs the device
kernels.  Inference only, exact fp32; there is no PyTorch fallback.  As in the reference, the output is NOT cropped: a
[B,3,H,W] input returns [B,3,Hp*scale,Wp*scale] with Hp, Wp the sides rounded up to a multiple of 16."""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._engine_module import EngineModule
from ..swinir.model import to_u8  # noqa: F401  (save_img1 is the same function in hat.py)
from .arch import RGB_MEAN, HATConfig, alias_of, buffer_value, is_buffer, state_schema, tap_names


class HAT(EngineModule):
    _family, _tap_names = 'hat', staticmethod(tap_names)

    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=(6, 6, 6, 6, 6, 6),
                 window_size=16, compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 use_checkpoint=False, upscale=2, img_range=1., upsampler='pixelshuffle', resi_connection='1conv', **kwargs):
        super().__init__()
        for what, ok in (("upsampler %r (only 'pixelshuffle')" % (upsampler,), upsampler == 'pixelshuffle'),
                         ("resi_connection %r (only '1conv')" % (resi_connection,), resi_connection == '1conv'),
                         ('patch_size %r (only 1)' % (patch_size,), patch_size == 1), ('ape=True', not ape),
                         ('in_chans %r (only 3)' % (in_chans,), in_chans == 3), ('qkv_bias=False', bool(qkv_bias)),
                         ('qk_scale %r (only None)' % (qk_scale,), qk_scale is None),
                         ('norm_layer %r (only nn.LayerNorm)' % (norm_layer,), norm_layer is nn.LayerNorm),
                         ('window_size %r (only 16)' % (window_size,), window_size == 16),
                         ('overlap_ratio %r (only 0.5)' % (overlap_ratio,), overlap_ratio == 0.5),
                         ('compress_ratio %r' % (compress_ratio,), isinstance(compress_ratio, int) and compress_ratio >= 1),
                         ('squeeze_factor %r' % (squeeze_factor,), isinstance(squeeze_factor, int) and squeeze_factor >= 1),
                         # at img_size <= window the reference shrinks the window and never shifts
                         ('img_size %r (must exceed the window)' % (img_size,), isinstance(img_size, int) and img_size > window_size),
                         ('upscale %r (only 2, 3, 4, 8)' % (upscale,), upscale in (2, 3, 4, 8))):
            if not ok:
                raise NotImplementedError('HAT on the HIP engine does not run ' + what)
        self.cfg = HATConfig(img_size, embed_dim, list(depths), list(num_heads), window_size, compress_ratio, squeeze_factor,
                             float(conv_scale), float(overlap_ratio), mlp_ratio, upscale, float(img_range), bool(patch_norm))
        self.upscale, self.window_size, self.img_range = upscale, window_size, img_range
        self.schema = state_schema(self.cfg)
        # dotted names cannot be registered on an nn.Module: the tensors live under p<i> and state_dict / load_state_dict speak
        # the reference's keys.  An aliased key (upsample.upsampling.2.*) has no tensor of its own: it is p<i> of the key it
        # repeats, as in the reference, where one Conv2d sits at several places of the list.
        self._names = list(self.schema)
        self._slot = {}
        for i, (k, shape) in enumerate(self.schema.items()):
            if alias_of(k) != k:
                self._slot[k] = self._slot[alias_of(k)]
                continue
            self._slot[k] = 'p%d' % i
            if is_buffer(k):
                self.register_buffer('p%d' % i, torch.from_numpy(buffer_value(self.cfg, k)))
            else:
                self.register_parameter('p%d' % i, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._init_engine()     # refuses what the kernels do not cover (head_dim, embed_dim, ...) with the library's message

    # ---- the reference's keys ----
    def _tensor(self, i, k):
        return getattr(self, self._slot[k])

    def _is_buffer(self, k):
        return is_buffer(k)

    def _buffer_differs(self, src, p):
        return tuple(src.shape) != tuple(p.shape) or not torch.equal(src.to(p.device, p.dtype), p)

    def _repeats(self, k, key, src, state_dict, prefix, error_msgs):
        first = prefix + alias_of(k)
        if alias_of(k) == k or first not in state_dict:
            return False
        # the reference holds ONE tensor under these keys
        if not torch.equal(src, state_dict[first]):
            error_msgs.append('%s differs from %s: the reference runs one shared convolution in every upsampling stage, '
                              'its state_dict repeats one tensor' % (key, first))
        return True

    def named_reference_parameters(self):
        return [(k, getattr(self, self._slot[k])) for k in self._names if not is_buffer(k) and alias_of(k) == k]

    # ---- the engine ----
    def _fill_config(self):
        cfg = self.cfg
        if len(cfg.depths) > _lib.FDSR_HAT_MAX_LAYERS:
            raise NotImplementedError('at most %d layers' % _lib.FDSR_HAT_MAX_LAYERS)
        c = _lib.FdsrHatConfig()
        c.embed_dim, c.n_layers, c.window_size, c.mlp_hidden = cfg.embed_dim, len(cfg.depths), cfg.window_size, cfg.mlp_hidden
        c.upscale, c.patch_norm, c.img_range = cfg.upscale, int(cfg.patch_norm), cfg.img_range
        c.compress_ratio, c.squeeze_factor, c.conv_scale = cfg.compress_ratio, cfg.squeeze_factor, cfg.conv_scale
        c.overlap_win_size = cfg.overlap_win_size
        for i, (d, h) in enumerate(zip(cfg.depths, cfg.num_heads)):
            c.depths[i], c.num_heads[i] = d, h
        for i in range(3):
            c.mean[i] = RGB_MEAN[i]
        return c

    @staticmethod
    def _check(x):
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.shape[1] == 3):
            raise ValueError('HAT takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        return x.float().contiguous()

    def padded(self, h, w):
        ws = self.window_size
        return -(-h // ws) * ws, -(-w // ws) * ws

    def output_shape(self, b, h, w):
        """The padded size times the scale: the reference does not crop."""
        hp, wp = self.padded(h, w)
        return (b, 3, hp * self.upscale, wp * self.upscale)

    def _debug_capacity(self, b, h, w):
        hp, wp = self.padded(h, w)
        return b * hp * wp * self.upscale ** 2 * max(self.cfg.embed_dim, 64)


def load_synthetic(model, seed=0):
    """Fill a HAT with synth.synth_hat's weights (tests, timing, smoke runs)."""
    from ..synth import synth_hat
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth_hat(model.cfg, seed).items()}
    model.load_state_dict(sd, strict=False)
    return model
