"""The checkpoint schema of HAT as MSI_SR_model/model/hat.py builds it (GeneratorResNet, upsampler='pixelshuffle',
resi_connection='1conv', patch_size 1, ape=False, three channels): every state_dict key and shape in state_dict order, the two
index buffers that are functions of the geometry, the aliased keys of the shared upsampling convolution, and the tap names of
fdsr_hat_debug_tensor.  csrc/fdsr_hat.hip takes the parameters under these names."""
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List

import numpy as np

from ..swinir.arch import NUM_FEAT, RGB_MEAN, attn_mask, region_ids, relative_position_index  # noqa: F401  (the SA index is SwinIR's formula)


@dataclass
class HATConfig:
    img_size: int = 64                     # sizes nothing: the mask is made for the padded input at forward time
    embed_dim: int = 180
    depths: List[int] = field(default_factory=lambda: [6] * 6)
    num_heads: List[int] = field(default_factory=lambda: [6] * 6)
    window_size: int = 16
    compress_ratio: int = 3
    squeeze_factor: int = 30
    conv_scale: float = 0.01
    overlap_ratio: float = 0.5
    mlp_ratio: float = 4.
    upscale: int = 2
    img_range: float = 1.
    patch_norm: bool = True

    @property
    def mlp_hidden(self):
        return int(self.embed_dim * self.mlp_ratio)

    @property
    def shift(self):
        return self.window_size // 2

    @property
    def overlap_win_size(self):
        return int(self.window_size * self.overlap_ratio) + self.window_size

    def upsample_convs(self):
        """(index inside Upsample.upsampling, factor) of every convolution that runs.  At x4 and x8 the reference's list holds the
        SAME Conv2d at every even index."""
        if self.upscale == 3:
            return [(0, 3)]
        return [(2 * k, 2) for k in range(int(self.upscale).bit_length() - 1)]


def relative_position_index_oca(ws, wse):
    """[ws*ws, wse*wse] as calculate_rpi_oca leaves it: ((ky - qy) + ws - wse + 1) * (ws + wse - 1) + (kx - qx) + ws - wse + 1,
    NEGATIVE for keys up and left of the query (-880 .. 640 at 16 / 24); indexing wraps those round the table."""
    qy, qx = np.divmod(np.arange(ws * ws), ws)
    ky, kx = np.divmod(np.arange(wse * wse), wse)
    off = ws - wse + 1
    return ((ky[None, :] - qy[:, None] + off) * (ws + wse - 1) + (kx[None, :] - qx[:, None] + off)).astype(np.int64)


def oca_table_rows(ws, wse):
    """The row of the (ws + wse - 1)^2 table that pairs query i with key j: the index above, wrapped."""
    return relative_position_index_oca(ws, wse) % ((ws + wse - 1) ** 2)


def _wb(out, name, *wshape):
    out[name + '.weight'] = tuple(wshape)
    out[name + '.bias'] = (wshape[0],)


def state_schema(cfg: HATConfig) -> "OrderedDict[str, tuple]":
    """Every state_dict entry, buffers and aliased keys included, in the reference's order."""
    c, ws, wse = cfg.embed_dim, cfg.window_size, cfg.overlap_win_size
    if len(cfg.depths) != len(cfg.num_heads):
        raise ValueError('depths and num_heads must have the same length')
    out = OrderedDict()
    out['relative_position_index_SA'] = (ws * ws, ws * ws)
    out['relative_position_index_OCA'] = (ws * ws, wse * wse)
    _wb(out, 'conv_first', c, 3, 3, 3)
    if cfg.patch_norm:
        _wb(out, 'patch_embed.norm', c)
    for i, (depth, heads) in enumerate(zip(cfg.depths, cfg.num_heads)):
        g = f'layers.{i}.residual_group'
        for j in range(depth):
            b = f'{g}.blocks.{j}'
            _wb(out, b + '.norm1', c)
            out[b + '.attn.relative_position_bias_table'] = ((2 * ws - 1) ** 2, heads)
            _wb(out, b + '.attn.qkv', 3 * c, c)
            _wb(out, b + '.attn.proj', c, c)
            _wb(out, b + '.conv_block.cab.0', c // cfg.compress_ratio, c, 3, 3)
            _wb(out, b + '.conv_block.cab.2', c, c // cfg.compress_ratio, 3, 3)
            _wb(out, b + '.conv_block.cab.3.attention.1', c // cfg.squeeze_factor, c, 1, 1)
            _wb(out, b + '.conv_block.cab.3.attention.3', c, c // cfg.squeeze_factor, 1, 1)
            _wb(out, b + '.norm2', c)
            _wb(out, b + '.mlp.fc1', cfg.mlp_hidden, c)
            _wb(out, b + '.mlp.fc2', c, cfg.mlp_hidden)
        o = g + '.overlap_attn'
        out[o + '.relative_position_bias_table'] = ((ws + wse - 1) ** 2, heads)
        _wb(out, o + '.norm1', c)
        _wb(out, o + '.qkv', 3 * c, c)
        _wb(out, o + '.proj', c, c)
        _wb(out, o + '.norm2', c)
        _wb(out, o + '.mlp.fc1', cfg.mlp_hidden, c)
        _wb(out, o + '.mlp.fc2', c, cfg.mlp_hidden)
        _wb(out, f'layers.{i}.conv', c, c, 3, 3)
    _wb(out, 'norm', c)
    _wb(out, 'conv_after_body', c, c, 3, 3)
    _wb(out, 'conv_before_upsample.0', NUM_FEAT, c, 3, 3)
    for idx, r in cfg.upsample_convs():
        _wb(out, f'upsample.upsampling.{idx}', r * r * NUM_FEAT, NUM_FEAT, 3, 3)
    _wb(out, 'conv_last', 3, NUM_FEAT, 3, 3)
    return out


def is_buffer(key):
    return key.startswith('relative_position_index_')


def alias_of(key):
    """The key whose tensor `key` shares: upsample.upsampling.{2,4}.* are upsample.upsampling.0.* again; every other key is its
    own."""
    parts = key.split('.')
    if key.startswith('upsample.upsampling.') and parts[2] != '0':
        return '.'.join(parts[:2] + ['0'] + parts[3:])
    return key


def param_schema(cfg: HATConfig) -> "OrderedDict[str, tuple]":
    """The parameters the engine holds: no buffers, one entry for the shared upsampling convolution."""
    return OrderedDict((k, s) for k, s in state_schema(cfg).items() if not is_buffer(k) and alias_of(k) == k)


def buffer_value(cfg: HATConfig, key):
    """What the geometry gives for a buffer of state_schema."""
    if key == 'relative_position_index_SA':
        return relative_position_index(cfg.window_size)
    return relative_position_index_oca(cfg.window_size, cfg.overlap_win_size)


def tap_names(cfg: HATConfig):
    """The named taps of fdsr_hat_debug_tensor, in execution order."""
    names = ['conv_first', 'patch_embed.norm']
    for i, depth in enumerate(cfg.depths):
        for j in range(depth):
            names += [f'layers.{i}.blocks.{j}.cab', f'layers.{i}.blocks.{j}.attn', f'layers.{i}.blocks.{j}.mlp']
        names += [f'layers.{i}.ocab.attn', f'layers.{i}.ocab.mlp', f'layers.{i}']
    names.append('conv_after_body')
    return names + [f'upsample.{k}' for k in range(len(cfg.upsample_convs()))]
