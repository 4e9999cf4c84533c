"""SwinIR on the HIP engine (include/fdsr.h: fdsr_swinir_*): an nn.Module that takes the constructor arguments of the
reference's GeneratorResNet (MSI_SR_model/model/swinir.py), owns its parameters and buffers under the reference's names --
`generator_param.pkl` loads with load_state_dict(strict=True) -- and whose forward runs the device kernels.  Inference only,
exact fp32; there is no PyTorch fallback."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._engine_module import EngineModule, _ptr
from .arch import RGB_MEAN, SwinIRConfig, buffer_value, is_buffer, state_schema, tap_names


class SwinIR(EngineModule):
    _family, _tap_names = 'swinir', staticmethod(tap_names)

    def __init__(self, img_size=256, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7,
                 mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm,
                 ape=False, patch_norm=True, use_checkpoint=False, upscale=4, img_range=1., upsampler='pixelshuffle',
                 resi_connection='1conv', **kwargs):
        super().__init__()
        for what, ok in (("upsampler %r (only 'pixelshuffle')" % (upsampler,), upsampler == 'pixelshuffle'),
                         ("resi_connection %r (only '1conv')" % (resi_connection,), resi_connection == '1conv'),
                         ('patch_size %r (only 1)' % (patch_size,), patch_size == 1), ('ape=True', not ape),
                         ('in_chans %r (only 3)' % (in_chans,), in_chans == 3), ('qkv_bias=False', bool(qkv_bias)),
                         ('qk_scale %r (only None)' % (qk_scale,), qk_scale is None),
                         ('norm_layer %r (only nn.LayerNorm)' % (norm_layer,), norm_layer is nn.LayerNorm),
                         ('window_size %r (only 8)' % (window_size,), window_size == 8),
                         # at img_size <= window the reference shrinks the window and never shifts
                         ('img_size %r (must exceed the window)' % (img_size,), isinstance(img_size, int) and img_size > window_size),
                         ('upscale %r (only 2, 3, 4, 8)' % (upscale,), upscale in (2, 3, 4, 8))):
            if not ok:
                raise NotImplementedError('SwinIR on the HIP engine does not run ' + what)
        self.cfg = SwinIRConfig(img_size, embed_dim, list(depths), list(num_heads), window_size, mlp_ratio, upscale, float(img_range),
                                bool(patch_norm))
        self.upscale, self.window_size, self.img_range = upscale, window_size, img_range
        self.schema = state_schema(self.cfg)
        # dotted names cannot be registered on an nn.Module: the tensors live under p<i> and state_dict / load_state_dict speak
        # the reference's keys
        self._names = list(self.schema)
        for i, (k, shape) in enumerate(self.schema.items()):
            if is_buffer(k):
                self.register_buffer('p%d' % i, torch.from_numpy(buffer_value(self.cfg, k)))
            else:
                self.register_parameter('p%d' % i, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._init_engine()     # refuses what the kernels do not cover (head_dim, embed_dim) with the library's message

    # ---- the reference's keys ----
    def _is_buffer(self, k):
        return is_buffer(k)

    def _buffer_differs(self, src, p):
        # checked where the sizes match (an attn_mask of another img_size is the same function at another size)
        return tuple(src.shape) == tuple(p.shape) and not torch.equal(src.to(p.device, p.dtype), p)

    def named_reference_parameters(self):
        return [(k, getattr(self, 'p%d' % i)) for i, k in enumerate(self._names) if not is_buffer(k)]

    # ---- the engine ----
    def _fill_config(self):
        cfg = self.cfg
        if len(cfg.depths) > _lib.FDSR_SWINIR_MAX_LAYERS:
            raise NotImplementedError('at most %d layers' % _lib.FDSR_SWINIR_MAX_LAYERS)
        c = _lib.FdsrSwinirConfig()
        c.embed_dim, c.n_layers, c.window_size, c.mlp_hidden = cfg.embed_dim, len(cfg.depths), cfg.window_size, cfg.mlp_hidden
        c.upscale, c.patch_norm, c.img_range = cfg.upscale, int(cfg.patch_norm), cfg.img_range
        for i, (d, h) in enumerate(zip(cfg.depths, cfg.num_heads)):
            c.depths[i], c.num_heads[i] = d, h
        for i in range(3):
            c.mean[i] = RGB_MEAN[i]
        return c

    @staticmethod
    def _check(x):
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.shape[1] == 3):
            raise ValueError('SwinIR takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        return x.float().contiguous()

    def output_shape(self, b, h, w):
        """The reference crops to the input's size times the scale."""
        return (b, 3, h * self.upscale, w * self.upscale)

    def _debug_capacity(self, b, h, w):
        pad = self.window_size
        hp, wp = -(-h // pad) * pad, -(-w // pad) * pad
        return b * hp * wp * self.upscale ** 2 * max(self.cfg.embed_dim, 64)


def to_u8(x):
    """The reference's save_img1 on the device: (x * 255).clamp(0, 255) truncated; [B,3,H,W] fp32 -> [B,H,W,3] uint8."""
    if not (x.is_cuda and x.dim() == 4 and x.shape[1] == 3):
        raise ValueError('to_u8 takes a [B,3,H,W] tensor on the GPU')
    x = x.float().contiguous()
    b, _, h, w = x.shape
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(None, _lib.load().fdsr_swinir_to_u8(_ptr(x), _ptr(out), b, h, w, C.c_void_p(st)))
    return out


def load_synthetic(model, seed=0):
    """Fill a SwinIR with synth.synth_swinir's weights (tests, timing, smoke runs)."""
    from ..synth import synth_swinir
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth_swinir(model.cfg, seed).items()}
    model.load_state_dict(sd, strict=False)
    return model
