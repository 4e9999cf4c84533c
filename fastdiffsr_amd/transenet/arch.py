"""The checkpoint schema of TransENet as MSI_SR_model/model/transenet.py builds it (class TransENet over model/transformer.py):
every state_dict key and shape in state_dict order, and the tap names of fdsr_transenet_debug_tensor.
csrc/fdsr_transenet.hip takes the parameters under these names."""
from collections import OrderedDict
from dataclasses import dataclass

# what TransENet.__init__ hard-codes
PATCH = 8
DIM = 512
HEADS = 6
DIM_HEAD = 32
INNER = HEADS * DIM_HEAD
MLP_DIM = 512
REDUCTION = 4
MIN_NUM_PATCHES = 12
RGB_MEAN = (0.4916, 0.4991, 0.4565)        # what sub_mean / add_mean are initialised from (UCMerced)
ENCODERS = ('encoder_stage1', 'encoder_stage2', 'encoder_stage3', 'encoder_up')
DECODERS = ('decoder1', 'decoder2', 'decoder3')     # state_dict order; they run 3, 2, 1


@dataclass
class TransENetConfig:
    n_feats: int = 64
    scale: int = 4
    n_colors: int = 3
    hr_patch_size: int = 256               # the HR height the inverse rearrange is called with: LR height = hr_patch_size / scale
    en_depth: int = 8
    de_depth: int = 1

    @property
    def channels(self):
        return self.n_feats // REDUCTION

    @property
    def patch_dim(self):
        return self.channels * PATCH * PATCH

    def upsample_convs(self):
        """(index inside the Upsampler, factor) of every convolution: a convolution of its own per stage."""
        if self.scale == 3:
            return [(0, 3)]
        return [(2 * k, 2) for k in range(int(self.scale).bit_length() - 1)]


def _wb(out, name, *wshape, bias=True):
    out[name + '.weight'] = tuple(wshape)
    if bias:
        out[name + '.bias'] = (wshape[0],)


def _attention(out, p):
    _wb(out, p + '.fn.norm', DIM)
    _wb(out, p + '.fn.fn.to_qkv', 3 * INNER, DIM, bias=False)
    _wb(out, p + '.fn.fn.to_out.0', DIM, INNER)


def _feed_forward(out, p):
    _wb(out, p + '.fn.norm', DIM)
    _wb(out, p + '.fn.fn.net.0', MLP_DIM, DIM)
    _wb(out, p + '.fn.fn.net.3', DIM, MLP_DIM)


def state_schema(cfg: TransENetConfig) -> "OrderedDict[str, tuple]":
    """Every state_dict entry in the reference's order (the order of the assignments in TransENet.__init__)."""
    nf, ch = cfg.n_feats, cfg.channels
    out = OrderedDict()
    _wb(out, 'sub_mean', 3, 3, 1, 1)
    _wb(out, 'head.0', nf, cfg.n_colors, 3, 3)
    for s in (1, 2, 3):
        for i in range(5):
            for j in (0, 2):
                _wb(out, f'feat_extrat_stage{s}.body.{i}.body.{j}', nf, nf, 3, 3)
    for name in ('stage1_conv1x1', 'stage2_conv1x1', 'stage3_conv1x1', 'up_conv1x1'):
        _wb(out, name, ch, nf, 1, 1)
    _wb(out, 'span_conv1x1', nf, ch, 1, 1)
    for idx, r in cfg.upsample_convs():
        _wb(out, f'upsampler.{idx}', r * r * nf, nf, 3, 3)
    _wb(out, 'tail', cfg.n_colors, nf, 3, 3)
    _wb(out, 'add_mean', 3, 3, 1, 1)
    for name in ('patch_to_embedding_low1', 'patch_to_embedding_low2', 'patch_to_embedding_low3', 'patch_to_embedding_high'):
        _wb(out, name, DIM, cfg.patch_dim)
    _wb(out, 'embedding_to_patch', cfg.patch_dim, DIM)
    for e in ENCODERS:
        for j in range(cfg.en_depth):
            _attention(out, f'{e}.layers.{j}.0')
            _feed_forward(out, f'{e}.layers.{j}.1')
    for d in DECODERS:
        for j in range(cfg.de_depth):
            _attention(out, f'{d}.layers.{j}.0')
            p = f'{d}.layers.{j}.1'
            _wb(out, p + '.fn.norm', DIM)
            for t in ('to_q', 'to_k', 'to_v'):
                _wb(out, f'{p}.fn.fn.{t}', INNER, DIM, bias=False)
            _wb(out, p + '.fn.fn.to_out.0', DIM, INNER)
            _feed_forward(out, f'{d}.layers.{j}.2')
    return out


def tap_names(cfg: TransENetConfig):
    """The named taps of fdsr_transenet_debug_tensor, in execution order.  Token tensors come back as [B, 512, h, w] with (h, w)
    the grid of 8 x 8 patches."""
    names = ['head']
    for s in (1, 2, 3):
        names += [f'stage{s}', f'stage{s}.1x1']
    names += ['up', 'up.1x1', 'embed.low1', 'embed.low2', 'embed.low3', 'embed.high']
    for e in ENCODERS:
        for j in range(cfg.en_depth):
            names += [f'{e}.{j}.attn', f'{e}.{j}.ff']
        names.append(e)
    for d in reversed(DECODERS):
        for j in range(cfg.de_depth):
            names += [f'{d}.{j}.self', f'{d}.{j}.cross', f'{d}.{j}.ff']
    return names + ['embedding_to_patch', 'span']
