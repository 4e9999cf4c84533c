"""Generate tests/golden/transenet.npz by RUNNING THE REFERENCE's TransENet (MSI_SR_model/model/transenet.py) on the CPU.

TEST INFRASTRUCTURE.  Runs only where the reference checkout exists (never on the GPU box).  The reference module is imported
for real, with stub modules around the import for what it pulls in and does not need for a forward pass (the stubs of
tools/make_hat_golden.py: torchvision, the old skimage.measure names, its own `utils` and `data` packages).  einops is the
installed one.  The network is built as main_transenet.py builds it (TransENet(n_feats, scale, n_basic_modules=10, n_colors=3,
hr_patch_size, back_projection_iters=10, en_depth, de_depth, conv=default_conv)), filled from
fastdiffsr_amd.synth.synth_transenet(cfg, SEED), put in eval mode and run in fp32; forward hooks record the taps.

The tool also checks transenet.arch against the reference: the state_dict keys in order and every shape.

The fixture holds DATA only: the seed, the inputs, the outputs and the taps (a tensor of more than GOLDEN_CAP elements as the
fixed sample tests/transenet_restatement.sample_index names).  No weights: the seed regenerates them.

Usage:  python tools/make_transenet_golden.py REFERENCE_DIR   (writes tests/golden/transenet.npz; REFERENCE_DIR holds MSI_SR_model/)
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
    sys.exit('usage: python tools/make_transenet_golden.py REFERENCE_DIR   (or FDSR_REFERENCE): the checkout that holds MSI_SR_model/')
OUT = os.path.join(ROOT, 'tests', 'golden', 'transenet.npz')

from fastdiffsr_amd.transenet.arch import state_schema  # noqa: E402
from fastdiffsr_amd.synth import synth_transenet  # noqa: E402
from transenet_restatement import CASES, GOLDEN_CASES, SEED, case_config, case_input, recorded_taps, sampled  # noqa: E402


def import_reference():
    def module(name, **attrs):
        m = sys.modules[name] = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

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
    sys.path.insert(0, os.path.join(REF, 'MSI_SR_model'))
    from model import transenet as ref
    return ref


def run_case(ref, name, out):
    base, scale, batch, hw, with_taps, _ = CASES[name]
    cfg = case_config(name)
    net = ref.TransENet(n_feats=cfg.n_feats, scale=scale, n_basic_modules=10, n_colors=3, hr_patch_size=cfg.hr_patch_size,
                        back_projection_iters=10, en_depth=cfg.en_depth, de_depth=cfg.de_depth, conv=ref.default_conv)
    # the schema against the reference's own state dict
    sd = net.state_dict()
    schema = state_schema(cfg)
    assert list(sd) == list(schema), [(a, b) for a, b in zip(sd, schema) if a != b][:4]
    for k, shape in schema.items():
        assert tuple(sd[k].shape) == tuple(shape), (k, tuple(sd[k].shape), shape)
    torch.nn.Module.load_state_dict(net, {k: torch.from_numpy(v) for k, v in synth_transenet(cfg, SEED).items()}, strict=True)
    net.eval()

    x = case_input(name, batch, hw[0], hw[1])
    low, high = (hw[0] // 8, hw[1] // 8), (hw[0] * scale // 8, hw[1] * scale // 8)
    taps = {}
    hooks = []

    def keep(tap, pick=lambda i, o: o):
        return lambda mod, inp, o=None: taps.__setitem__(tap, pick(inp, o).detach().clone())

    def tokens(grid):
        return lambda i, o: o.reshape(o.shape[0], grid[0], grid[1], -1).permute(0, 3, 1, 2)

    if with_taps:
        hooks.append(net.head.register_forward_hook(keep('head')))
        for s in (1, 2, 3):
            hooks.append(getattr(net, f'feat_extrat_stage{s}').register_forward_hook(keep(f'stage{s}')))
            hooks.append(getattr(net, f'stage{s}_conv1x1').register_forward_hook(keep(f'stage{s}.1x1')))
            hooks.append(getattr(net, f'patch_to_embedding_low{s}').register_forward_hook(keep(f'embed.low{s}', tokens(low))))
        hooks.append(net.upsampler.register_forward_hook(keep('up')))
        hooks.append(net.up_conv1x1.register_forward_hook(keep('up.1x1')))
        hooks.append(net.patch_to_embedding_high.register_forward_hook(keep('embed.high', tokens(high))))
        for e, grid in (('encoder_stage1', low), ('encoder_stage2', low), ('encoder_stage3', low), ('encoder_up', high)):
            enc = getattr(net, e)
            for j, (attn, ff) in enumerate(enc.layers):
                hooks.append(attn.register_forward_hook(keep(f'{e}.{j}.attn', tokens(grid))))
                hooks.append(ff.register_forward_hook(keep(f'{e}.{j}.ff', tokens(grid))))
            hooks.append(enc.register_forward_hook(keep(e, tokens(grid))))
        for d in (1, 2, 3):
            for j, (a1, a2, ff) in enumerate(getattr(net, f'decoder{d}').layers):
                hooks.append(a1.register_forward_hook(keep(f'decoder{d}.{j}.self', tokens(high))))
                hooks.append(a2.register_forward_hook(keep(f'decoder{d}.{j}.cross', tokens(high))))
                hooks.append(ff.register_forward_hook(keep(f'decoder{d}.{j}.ff', tokens(high))))
        hooks.append(net.span_conv1x1.register_forward_pre_hook(keep('embedding_to_patch', lambda i, o: i[0])))
        hooks.append(net.span_conv1x1.register_forward_hook(keep('span')))
    with torch.no_grad():
        y = net(x)
    for h in hooks:
        h.remove()
    assert tuple(y.shape) == (batch, 3, hw[0] * scale, hw[1] * scale)
    out[name + '/x'] = x.numpy()
    out[name + '/out'] = sampled(name + '/out', y)
    if with_taps:
        for tap in recorded_taps(cfg):
            out[name + '/' + tap] = sampled(name + '/' + tap, taps[tap])
    print(f'{name}: x {tuple(x.shape)} -> out {tuple(y.shape)}, range [{float(y.min()):.3f}, {float(y.max()):.3f}], '
          f'{len(taps)} taps hooked', flush=True)


def main():
    ref = import_reference()
    out = {'seed': np.array(SEED), 'cases': np.array(sorted(GOLDEN_CASES))}
    for name in GOLDEN_CASES:
        run_case(ref, name, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
