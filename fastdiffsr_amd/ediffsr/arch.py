"""The checkpoint schema of EDiffSR's ConditionalNAFNet (DenoisingNAFNet_arch.py): every state_dict key and shape, in
state_dict order, for any width / enc_blk_nums / middle_blk_num / dec_blk_nums.  csrc/fdsr_nafnet.hip builds the same list
(fdsr_nafnet_weight_info); tests compare the two with each other and with the reference module's own state_dict."""
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List


@dataclass
class NAFNetConfig:
    img_channel: int = 3
    width: int = 64
    middle_blk_num: int = 1
    enc_blk_nums: List[int] = field(default_factory=lambda: [14, 1, 1, 1])
    dec_blk_nums: List[int] = field(default_factory=lambda: [1, 1, 1, 1])

    @property
    def padder_size(self):
        return 2 ** len(self.enc_blk_nums)


def _conv(out, name, cout, cin, k, bias=True):
    out[name + '.weight'] = (cout, cin, k, k)
    if bias:
        out[name + '.bias'] = (cout,)


def _block(out, name, c, width):
    # parameters first (beta, gamma), then the sub-modules in the order NAFBlock.__init__ registers them
    out[name + '.beta'] = (1, c, 1, 1)
    out[name + '.gamma'] = (1, c, 1, 1)
    out[name + '.mlp.1.weight'] = (4 * c, 2 * width)
    out[name + '.mlp.1.bias'] = (4 * c,)
    _conv(out, name + '.conv1', 2 * c, c, 1)
    _conv(out, name + '.conv2', 2 * c, 1, 3)
    _conv(out, name + '.conv3', c, c, 1)
    _conv(out, name + '.sca.1', c, c, 1)
    _conv(out, name + '.conv4', 2 * c, c, 1)
    _conv(out, name + '.conv5', c, c, 1)
    out[name + '.norm1.g'] = (1, c, 1, 1)
    out[name + '.norm2.g'] = (1, c, 1, 1)


def param_schema(cfg: NAFNetConfig) -> "OrderedDict[str, tuple]":
    w = cfg.width
    if len(cfg.enc_blk_nums) != len(cfg.dec_blk_nums):
        raise ValueError('enc_blk_nums and dec_blk_nums must have the same length')
    out = OrderedDict()
    out['time_mlp.1.weight'] = (8 * w, w)
    out['time_mlp.1.bias'] = (8 * w,)
    out['time_mlp.3.weight'] = (4 * w, 4 * w)
    out['time_mlp.3.bias'] = (4 * w,)
    _conv(out, 'intro', w, 2 * cfg.img_channel, 3)
    _conv(out, 'enhance.rcab.0', w, w, 3)
    _conv(out, 'enhance.rcab.2', w, w, 3)
    _conv(out, 'enhance.rcab.3.attention.1', w // 16, w, 1)
    _conv(out, 'enhance.rcab.3.attention.3', w, w // 16, 1)
    _conv(out, 'ending', cfg.img_channel, w, 3)
    chan = w
    for i, num in enumerate(cfg.enc_blk_nums):
        for j in range(num):
            _block(out, f'encoders.{i}.{j}', chan, w)
        chan *= 2
    mid = chan
    for i, num in enumerate(cfg.dec_blk_nums):
        chan //= 2
        for j in range(num):
            _block(out, f'decoders.{i}.{j}', chan, w)
    for j in range(cfg.middle_blk_num):
        _block(out, f'middle_blks.{j}', mid, w)
    chan = mid
    for i in range(len(cfg.dec_blk_nums)):
        _conv(out, f'ups.{i}.0', 2 * chan, chan, 1, bias=False)
        chan //= 2
    chan = w
    for i in range(len(cfg.enc_blk_nums)):
        _conv(out, f'downs.{i}', 2 * chan, chan, 2)
        chan *= 2
    return out


def tap_names(cfg: NAFNetConfig):
    """The named taps of fdsr_nafnet_debug_tensor, in execution order."""
    names = ['intro', 'enhance']
    for i, num in enumerate(cfg.enc_blk_nums):
        names += [f'encoders.{i}.{j}' for j in range(num)] + [f'downs.{i}']
    names += [f'middle_blks.{j}' for j in range(cfg.middle_blk_num)]
    for i, num in enumerate(cfg.dec_blk_nums):
        names += [f'ups.{i}'] + [f'decoders.{i}.{j}' for j in range(num)]
    return names + ['ending']
