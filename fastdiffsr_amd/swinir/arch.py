"""The checkpoint schema of SwinIR as MSI_SR_model/model/swinir.py builds it (GeneratorResNet, upsampler='pixelshuffle',
resi_connection='1conv', patch_size 1, ape=False, three channels): every state_dict key and shape in state_dict order, the
two buffer kinds (attn.relative_position_index, attn_mask) that are functions of the geometry, and the tap names of
fdsr_swinir_debug_tensor.  csrc/fdsr_swinir.hip takes the parameters under these names."""
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List

import numpy as np

NUM_FEAT = 64                              # channels of the reconstruction tail
RGB_MEAN = (0.4488, 0.4371, 0.4040)


@dataclass
class SwinIRConfig:
    img_size: int = 64                     # sizes the attn_mask buffers only; any input size runs
    embed_dim: int = 180
    depths: List[int] = field(default_factory=lambda: [6] * 6)
    num_heads: List[int] = field(default_factory=lambda: [6] * 6)
    window_size: int = 8
    mlp_ratio: float = 2.
    upscale: int = 4
    img_range: float = 1.
    patch_norm: bool = True

    @property
    def mlp_hidden(self):
        return int(self.embed_dim * self.mlp_ratio)

    @property
    def shift(self):
        return self.window_size // 2

    def upsample_convs(self):
        """(index inside nn.Sequential, factor) of every conv of Upsample: one per factor of two, one of 3 at scale 3."""
        if self.upscale == 3:
            return [(0, 3)]
        return [(2 * k, 2) for k in range(int(self.upscale).bit_length() - 1)]


def relative_position_index(ws):
    """[ws*ws, ws*ws]: the row of relative_position_bias_table that pairs query i with key j."""
    y, x = np.divmod(np.arange(ws * ws), ws)
    return ((y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)).astype(np.int64)


def region_ids(h, w, ws, shift):
    """[h, w]: the region of every pixel of the rolled image -- three slices per axis, [0, n - ws), [n - ws, n - shift), [n - shift, n)."""
    def axis(n):
        i = np.arange(n)
        return (i >= n - ws).astype(np.int64) + (i >= n - shift)
    return axis(h)[:, None] * 3 + axis(w)[None, :]


def attn_mask(h, w, ws, shift):
    """[nW, ws*ws, ws*ws] fp32: -100 between tokens of different regions, 0 elsewhere; windows row-major."""
    ids = region_ids(h, w, ws, shift).reshape(h // ws, ws, w // ws, ws).transpose(0, 2, 1, 3).reshape(-1, ws * ws)
    return np.where(ids[:, None, :] != ids[:, :, None], np.float32(-100.0), np.float32(0.0))


def _wb(out, name, *wshape):
    out[name + '.weight'] = tuple(wshape)
    out[name + '.bias'] = (wshape[0],)


def state_schema(cfg: SwinIRConfig) -> "OrderedDict[str, tuple]":
    """Every state_dict entry, buffers included, in the reference's order (a module's own parameters, its own buffers, then
    its children in registration order)."""
    c, ws = cfg.embed_dim, cfg.window_size
    if len(cfg.depths) != len(cfg.num_heads):
        raise ValueError('depths and num_heads must have the same length')
    n_win = (cfg.img_size // ws) ** 2
    out = OrderedDict()
    _wb(out, 'conv_first', c, 3, 3, 3)
    if cfg.patch_norm:
        _wb(out, 'patch_embed.norm', c)
    for i, (depth, heads) in enumerate(zip(cfg.depths, cfg.num_heads)):
        for j in range(depth):
            b = f'layers.{i}.residual_group.blocks.{j}'
            if j % 2:
                out[b + '.attn_mask'] = (n_win, ws * ws, ws * ws)
            _wb(out, b + '.norm1', c)
            out[b + '.attn.relative_position_bias_table'] = ((2 * ws - 1) ** 2, heads)
            out[b + '.attn.relative_position_index'] = (ws * ws, ws * ws)
            _wb(out, b + '.attn.qkv', 3 * c, c)
            _wb(out, b + '.attn.proj', c, c)
            _wb(out, b + '.norm2', c)
            _wb(out, b + '.mlp.fc1', cfg.mlp_hidden, c)
            _wb(out, b + '.mlp.fc2', c, cfg.mlp_hidden)
        _wb(out, f'layers.{i}.conv', c, c, 3, 3)
    _wb(out, 'norm', c)
    _wb(out, 'conv_after_body', c, c, 3, 3)
    _wb(out, 'conv_before_upsample.0', NUM_FEAT, c, 3, 3)
    for idx, r in cfg.upsample_convs():
        _wb(out, f'upsample.{idx}', r * r * NUM_FEAT, NUM_FEAT, 3, 3)
    _wb(out, 'conv_last', 3, NUM_FEAT, 3, 3)
    return out


def is_buffer(key):
    return key.endswith(('.attn_mask', '.relative_position_index'))


def param_schema(cfg: SwinIRConfig) -> "OrderedDict[str, tuple]":
    """The parameters: what the engine loads."""
    return OrderedDict((k, s) for k, s in state_schema(cfg).items() if not is_buffer(k))


def buffer_value(cfg: SwinIRConfig, key):
    """What the geometry gives for a buffer of state_schema."""
    if key.endswith('.relative_position_index'):
        return relative_position_index(cfg.window_size)
    return attn_mask(cfg.img_size, cfg.img_size, cfg.window_size, cfg.shift)


def tap_names(cfg: SwinIRConfig):
    """The named taps of fdsr_swinir_debug_tensor, in execution order."""
    names = ['conv_first', 'patch_embed.norm']
    for i, depth in enumerate(cfg.depths):
        for j in range(depth):
            names += [f'layers.{i}.blocks.{j}.attn', f'layers.{i}.blocks.{j}.mlp']
        names.append(f'layers.{i}')
    names.append('conv_after_body')
    return names + [f'upsample.{k}' for k in range(len(cfg.upsample_convs()))]
