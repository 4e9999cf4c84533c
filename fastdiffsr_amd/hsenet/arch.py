"""The checkpoint schema of HSENet as MSI_SR_model/model/hsenet.py builds it (class HSENET): every state_dict key and shape in
state_dict order, and the tap names of fdsr_hsenet_debug_tensor.  csrc/fdsr_hsenet.hip takes the parameters under these names."""
from collections import OrderedDict
from dataclasses import dataclass

RGB_MEAN = (0.4916, 0.4991, 0.4565)        # what sub_mean / add_mean are initialised from (UCMerced); rgb_std is 1
NONLOCAL = ('g', 'W', 'theta', 'phi')      # the order NonLocalBlock2D and AdjustedNonLocalBlock assign them in


@dataclass
class HSENetConfig:
    n_feats: int = 64
    scale: int = 3
    n_colors: int = 3
    n_basic_modules: int = 10

    @property
    def inter(self):
        """Channels of theta, phi and g: the one head of every non-local block."""
        return self.n_feats // 2

    def upsample_convs(self):
        """(index inside the Upsampler, factor) of every convolution: conv + PixelShuffle per stage."""
        if self.scale == 3:
            return [(0, 3)]
        return [(2 * k, 2) for k in range(int(self.scale).bit_length() - 1)]


def _wb(out, name, *wshape):
    out[name + '.weight'] = tuple(wshape)
    out[name + '.bias'] = (wshape[0],)


def _nonlocal(out, p, nf):
    for t in NONLOCAL:
        if t == 'W':
            _wb(out, f'{p}.W', nf, nf // 2, 1, 1)
        else:
            _wb(out, f'{p}.{t}', nf // 2, nf, 1, 1)


def _ssem(out, p, nf):
    for name in ('head.0.0', 'MB.0.0', 'MB.1.0'):
        _wb(out, f'{p}.{name}', nf, nf, 3, 3)
    _nonlocal(out, p + '.AB.0', nf)
    _wb(out, p + '.AB.1', nf, nf, 1, 1)
    _wb(out, p + '.tail.0.0', nf, nf, 3, 3)


def state_schema(cfg: HSENetConfig) -> "OrderedDict[str, tuple]":
    """Every state_dict entry in the reference's order (the order of the assignments in each module's __init__)."""
    nf = cfg.n_feats
    out = OrderedDict()
    _wb(out, 'sub_mean', 3, 3, 1, 1)
    for i in range(cfg.n_basic_modules):
        p = f'body_modulist.{i}'
        _wb(out, p + '.head.0.0', nf, nf, 3, 3)
        _wb(out, p + '.head.1.0', nf, nf, 3, 3)
        _nonlocal(out, p + '.body.0.NonLocal_base', nf)
        _ssem(out, p + '.body.0.base_scale.0', nf)
        _ssem(out, p + '.body.0.down_scale.0', nf)
        _wb(out, p + '.body.0.tail.0.0', nf, nf, 3, 3)
        _wb(out, p + '.tail.0.0', nf, nf, 3, 3)
        _wb(out, p + '.tail.1.0', nf, nf, 3, 3)
    _wb(out, 'add_mean', 3, 3, 1, 1)
    _wb(out, 'head.0', nf, cfg.n_colors, 3, 3)
    for idx, r in cfg.upsample_convs():
        _wb(out, f'tail.0.{idx}', r * r * nf, nf, 3, 3)
    _wb(out, 'tail.1', cfg.n_colors, nf, 3, 3)
    return out


MODULE_TAPS = ('head', 'base.nl', 'base.gate', 'base', 'down.in', 'down.nl', 'down.gate', 'down', 'up', 'cross', 'hsem')


def tap_names(cfg: HSENetConfig):
    """The named taps of fdsr_hsenet_debug_tensor, in execution order.  Of BasicModule i: m{i}.head its two head blocks;
    m{i}.base.nl, .base.gate, .base the base SSEM's non-local block (AB.0), MB * sigmoid(AB) and output; m{i}.down.in the
    half-scale input, m{i}.down.* its SSEM (all at half scale); m{i}.up its upsampled output; m{i}.cross the
    AdjustedNonLocalBlock; m{i}.hsem the HSEM; m{i} the module.  head, body (after + head) and up (the Upsampler) frame them."""
    names = ['head']
    for i in range(cfg.n_basic_modules):
        names += [f'm{i}.{t}' for t in MODULE_TAPS] + [f'm{i}']
    return names + ['body', 'up']
