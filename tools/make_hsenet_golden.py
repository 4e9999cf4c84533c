"""Generate tests/golden/hsenet.npz by RUNNING THE REFERENCE's HSENET (MSI_SR_model/model/hsenet.py) on the CPU.

TEST INFRASTRUCTURE.  Runs only where the reference checkout exists (never on the GPU box).  The reference module is imported
for real, behind the stub modules of tools/make_transenet_golden.py for what it pulls in and does not need for a forward
pass.  The network is built as mfeNew_validateByClass builds it (HSENET(n_feats, scale, n_basic_modules)), filled from
fastdiffsr_amd.synth.synth_hsenet(cfg, SEED, the case's qk_gain), put in eval mode and run in fp32; forward hooks record the taps.

The tool also checks hsenet.arch against the reference: the state_dict keys in order and every shape.

The fixture holds DATA only: the seed, the inputs, the outputs and the taps (a tensor of more than GOLDEN_CAP elements as the
fixed sample tests/hsenet_restatement.sample_index names), and the schema's keys and shapes as the reference's state dict has
them.  No weights: the seed regenerates them.

Usage:  python tools/make_hsenet_golden.py REFERENCE_DIR   (writes tests/golden/hsenet.npz; REFERENCE_DIR holds MSI_SR_model/)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
if len(sys.argv) < 2 and not os.environ.get('FDSR_REFERENCE'):
    sys.exit('usage: python tools/make_hsenet_golden.py REFERENCE_DIR   (or FDSR_REFERENCE): the checkout that holds MSI_SR_model/')
OUT = os.path.join(ROOT, 'tests', 'golden', 'hsenet.npz')

from fastdiffsr_amd.hsenet.arch import HSENetConfig, state_schema  # noqa: E402
from hsenet_restatement import CASES, GOLDEN_CASES, SEED, case_config, case_input, case_weights, recorded_taps, sampled  # noqa: E402


def import_reference():
    """model.hsenet behind make_transenet_golden's stubs: that tool's import_reference installs them and the path (and imports
    model.transenet on the way)."""
    spec = importlib.util.spec_from_file_location('make_transenet_golden', os.path.join(ROOT, 'tools', 'make_transenet_golden.py'))
    te = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(te)
    te.import_reference()
    from model import hsenet as ref
    return ref


def run_case(ref, name, out):
    _, _, scale, batch, hw, with_taps, _ = CASES[name]
    cfg = case_config(name)
    net = ref.HSENET(n_feats=cfg.n_feats, scale=scale, n_basic_modules=cfg.n_basic_modules)
    # the schema against the reference's own state dict
    sd = net.state_dict()
    schema = state_schema(cfg)
    assert list(sd) == list(schema), [(a, b) for a, b in zip(sd, schema) if a != b][:4]
    for k, shape in schema.items():
        assert tuple(sd[k].shape) == tuple(shape), (k, tuple(sd[k].shape), shape)
    torch.nn.Module.load_state_dict(net, {k: torch.from_numpy(v) for k, v in case_weights(name).items()}, strict=True)
    net.eval()

    x = case_input(name, batch, hw[0], hw[1])
    taps = {}
    hooks = []

    def keep(tap, pick=lambda i, o: o):
        return lambda mod, inp, o=None: taps.__setitem__(tap, pick(inp, o).detach().clone())

    def first(i, o):
        return i[0]

    if with_taps:
        hooks.append(net.head.register_forward_hook(keep('head')))
        for i, bm in enumerate(net.body_modulist):
            tp = f'm{i}'
            hsem = bm.body[0]
            hooks.append(bm.head.register_forward_hook(keep(tp + '.head')))
            for which, ssem in (('base', hsem.base_scale[0]), ('down', hsem.down_scale[0])):
                hooks.append(ssem.AB[0].register_forward_hook(keep(f'{tp}.{which}.nl')))
                hooks.append(ssem.tail.register_forward_pre_hook(keep(f'{tp}.{which}.gate', first)))
                hooks.append(ssem.register_forward_hook(keep(f'{tp}.{which}')))
            hooks.append(hsem.down_scale.register_forward_pre_hook(keep(tp + '.down.in', first)))
            hooks.append(hsem.NonLocal_base.register_forward_pre_hook(keep(tp + '.up', lambda i, o: i[1])))
            hooks.append(hsem.NonLocal_base.register_forward_hook(keep(tp + '.cross')))
            hooks.append(hsem.register_forward_hook(keep(tp + '.hsem')))
            hooks.append(bm.register_forward_hook(keep(tp)))
        hooks.append(net.tail[0].register_forward_pre_hook(keep('body', first)))
        hooks.append(net.tail[0].register_forward_hook(keep('up')))
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
    return net


def main():
    ref = import_reference()
    out = {'seed': np.array(SEED), 'cases': np.array(sorted(GOLDEN_CASES))}
    for name in GOLDEN_CASES:
        net = run_case(ref, name, out)
    # the reference's configuration (the last case's): the state dict's keys and shapes, for the host test of arch.state_schema
    sd = net.state_dict()
    assert case_config(GOLDEN_CASES[-1]) == HSENetConfig(64, 4, 3, 10)
    out['schema/keys'] = np.array(list(sd))
    out['schema/shapes'] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    out['schema/params'] = np.array(sum(v.numel() for v in sd.values()))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
