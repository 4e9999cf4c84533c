"""Generate tests/golden/hat.npz by RUNNING THE REFERENCE's GeneratorResNet (MSI_SR_model/model/hat.py) on the CPU.

TEST INFRASTRUCTURE.  Runs only where the reference checkout exists (never on the GPU box).  The reference module is imported
for real, with stub modules around the import for what it pulls in and does not need for a forward pass: torchvision, the old
skimage.measure names, its own `utils` and `data` packages, and timm.models.layers, whose three names are given their usual
meaning (to_2tuple, torch's trunc_normal_, DropPath as the identity of eval mode).  einops is the installed one.  The network
is filled from fastdiffsr_amd.synth.synth_hat(cfg, SEED), put in eval mode and run in fp32; forward hooks record the taps.

The tool also checks hat.arch against the reference: the state_dict keys in order, every shape, the two index buffers, and
that the upsampling keys the schema calls aliases are one tensor in the reference.

The fixture holds DATA only: the seed, the inputs, the outputs and the taps (a tensor of more than 8192 elements as the fixed
sample tests/hat_restatement.sample_index names).  No weights: the seed regenerates them.

Usage:  python tools/make_hat_golden.py REFERENCE_DIR      (writes tests/golden/hat.npz; REFERENCE_DIR holds MSI_SR_model/)
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('FDSR_REFERENCE')
if not REF:
    sys.exit('usage: python tools/make_hat_golden.py REFERENCE_DIR   (or FDSR_REFERENCE): the checkout that holds MSI_SR_model/')
OUT = os.path.join(ROOT, 'tests', 'golden', 'hat.npz')

from fastdiffsr_amd.hat.arch import HATConfig, alias_of, buffer_value, is_buffer, state_schema, tap_names  # noqa: E402
from fastdiffsr_amd.synth import synth_hat  # noqa: E402
from hat_restatement import CASES, GOLDEN_CASES, SEED, case_input, recorded_taps, sampled  # noqa: E402


def import_reference():
    def module(name, **attrs):
        m = sys.modules[name] = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    class DropPath(torch.nn.Module):
        def __init__(self, drop_prob=None):
            super().__init__()
            self.drop_prob = drop_prob

        def forward(self, x):
            assert not self.training
            return x

    tv = module('torchvision')
    tv.transforms = module('torchvision.transforms', ToPILImage=None, ToTensor=None)
    tv.utils = module('torchvision.utils', save_image=None)
    tv.datasets = module('torchvision.datasets')
    tv.models = module('torchvision.models', vgg19=None)
    sk = module('skimage')
    sk.measure = module('skimage.measure', compare_ssim=None, compare_mse=None, compare_psnr=None, compare_nrmse=None)
    ut = module('utils')
    ut.utils = module('utils.utils')
    ut.logger = module('utils.logger', Logger=None, PrintLogger=None)
    da = module('data')
    da.data = module('data.data', get_training_datasets=None, get_test_datasets=None, get_RGB_trainDataset=None, get_RGB_testDataset=None)
    module('timm').models = module('timm.models')
    sys.modules['timm.models'].layers = module('timm.models.layers', DropPath=DropPath, trunc_normal_=torch.nn.init.trunc_normal_,
                                               to_2tuple=lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x, x))
    sys.path.insert(0, os.path.join(REF, 'MSI_SR_model'))
    from model import hat as ref
    return ref


def tokens_to_nchw(t, hw):
    return t.reshape(t.shape[0], hw[0], hw[1], -1).permute(0, 3, 1, 2)


def run_case(ref, name, base, upscale, hw, with_taps, out):
    cfg = HATConfig(upscale=upscale, **base)
    # every argument but those of the case at the reference's default, as main_hat.py builds it
    kw = {k: v for k, v in base.items() if k != 'img_size'}
    net = ref.GeneratorResNet(upscale=upscale, in_chans=3, img_size=cfg.img_size, **kw)
    # the schema against the reference's own state dict
    sd = net.state_dict()
    schema = state_schema(cfg)
    assert list(sd) == list(schema), [(a, b) for a, b in zip(sd, schema) if a != b][:4]
    for k, shape in schema.items():
        assert tuple(sd[k].shape) == tuple(shape), (k, tuple(sd[k].shape), shape)
        if is_buffer(k):
            assert np.array_equal(sd[k].numpy(), buffer_value(cfg, k)), k
        assert sd[k].data_ptr() == sd[alias_of(k)].data_ptr(), ('not one tensor', k)
    own = [k for k in schema if alias_of(k) == k]
    assert len({sd[k].data_ptr() for k in own}) == len(own), 'two keys that the schema keeps apart share a tensor'
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hat(cfg, SEED).items()}, strict=False)
    assert not unexpected and all(is_buffer(k) or alias_of(k) != k for k in missing), (missing, unexpected)
    net.eval()

    x = case_input(name, 1, hw[0], hw[1])
    pad = [-(-s // 16) * 16 for s in hw]
    taps = {}
    hooks = []

    def keep(tap, pick):
        return lambda mod, inp, o=None: taps.__setitem__(tap, pick(inp, o).detach().clone())

    if with_taps:
        hooks.append(net.conv_first.register_forward_hook(keep('conv_first', lambda i, o: o)))
        hooks.append(net.patch_embed.register_forward_hook(keep('patch_embed.norm', lambda i, o: tokens_to_nchw(o, pad))))
        for li, layer in enumerate(net.layers):
            for bj, blk in enumerate(layer.residual_group.blocks):
                hooks.append(blk.conv_block.register_forward_hook(keep(f'layers.{li}.blocks.{bj}.cab', lambda i, o: o)))
                hooks.append(blk.norm2.register_forward_pre_hook(keep(f'layers.{li}.blocks.{bj}.attn', lambda i, o: tokens_to_nchw(i[0], pad))))
                hooks.append(blk.register_forward_hook(keep(f'layers.{li}.blocks.{bj}.mlp', lambda i, o: tokens_to_nchw(o, pad))))
            oc = layer.residual_group.overlap_attn
            hooks.append(oc.norm2.register_forward_pre_hook(keep(f'layers.{li}.ocab.attn', lambda i, o: tokens_to_nchw(i[0], pad))))
            hooks.append(oc.register_forward_hook(keep(f'layers.{li}.ocab.mlp', lambda i, o: tokens_to_nchw(o, pad))))
            hooks.append(layer.register_forward_hook(keep(f'layers.{li}', lambda i, o: tokens_to_nchw(o, pad))))
        hooks.append(net.conv_before_upsample.register_forward_pre_hook(keep('conv_after_body', lambda i, o: i[0])))
        # ONE PixelShuffle module sits at every odd index of the list: its hook fires once per stage
        def keep_stage(mod, inp, o):
            taps['upsample.%d' % sum(t.startswith('upsample.') for t in taps)] = o.detach().clone()

        hooks.append(net.upsample.upsampling[1].register_forward_hook(keep_stage))
    with torch.no_grad():
        y = net(x)
    for h in hooks:
        h.remove()
    assert tuple(y.shape) == (1, 3, pad[0] * upscale, pad[1] * upscale)      # the reference does not crop
    out[name + '/x'] = x.numpy()
    out[name + '/out'] = sampled(name + '/out', y)
    if with_taps:
        for tap in recorded_taps(tap_names(cfg)):
            out[name + '/' + tap] = sampled(name + '/' + tap, taps[tap])
    print(f'{name}: x {tuple(x.shape)} -> out {tuple(y.shape)}, range [{float(y.min()):.3f}, {float(y.max()):.3f}], '
          f'{len(taps)} taps hooked', flush=True)


def main():
    ref = import_reference()
    out = {'seed': np.array(SEED), 'cases': np.array(sorted(GOLDEN_CASES))}
    for name in GOLDEN_CASES:
        base, upscale, hw, with_taps, _ = CASES[name]
        run_case(ref, name, base, upscale, hw, with_taps, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
