"""tests/golden/ediffsr.npz from the reference's OWN modules (EDiffSR/codes: DenoisingNAFNet_arch.ConditionalNAFNet,
utils/sde_utils.IRSDE), fp32 on the CPU.  It pins tests/ediffsr_restatement.py and fastdiffsr_amd/ediffsr/{arch,sde}.py to the
reference; it runs only where a checkout of the reference exists (REFERENCE_ROOT = its FastDiffSR folder; default: the one oracle/make_goldens.py reads) and never on the
GPU box.  torchvision is absent here and is stubbed (sde_utils imports torchvision.utils for image dumps only).

    REFERENCE_ROOT=/path/to/FastDiffSR python tools/make_ediffsr_golden.py

Contents: key / shape lists of two settings; the sha256 of the synthetic state dict (synth.synth_nafnet(0) -- the weights are
regenerated from the seed, not stored); inputs, output and a strided sample (every TAP_STRIDE-th element) of every named tap
of one forward at 36x44 with an int time; a 32x32 forward with per-image float times; the IR-SDE tables of three schedules at
(T 100, eps 0.005); the final states of a short SDE and ODE loop (T 10, eps 0.5); one bicubic upscale."""
import importlib
import importlib.util
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_goldens import REF as _ORACLE_REF   # noqa: E402  (the checkout the oracle's own recipe reads)
REF = os.environ.get('REFERENCE_ROOT') or _ORACLE_REF
CODES = os.path.join(REF, 'EDiffSR', 'codes')
OUT = os.path.join(ROOT, 'tests', 'golden', 'ediffsr.npz')
TAP_STRIDE = 53
TEST_SETTING = dict(width=16, enc_blk_nums=[2, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
SHIPPED_SETTING = dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def import_reference():
    tv, tvu = types.ModuleType('torchvision'), types.ModuleType('torchvision.utils')
    tv.utils = tvu
    sys.modules.setdefault('torchvision', tv)
    sys.modules.setdefault('torchvision.utils', tvu)
    pkg = types.ModuleType('ediffsr_ref_modules')          # the modules directory as a package, without running its __init__
    pkg.__path__ = [os.path.join(CODES, 'config', 'sisr', 'models', 'modules')]
    sys.modules['ediffsr_ref_modules'] = pkg
    arch = importlib.import_module('ediffsr_ref_modules.DenoisingNAFNet_arch')
    spec = importlib.util.spec_from_file_location('ediffsr_ref_sde_utils', os.path.join(CODES, 'utils', 'sde_utils.py'))
    sde_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sde_utils)
    return arch, sde_utils


def inputs(seed, b, h, w):
    g = torch.Generator().manual_seed(seed)
    cond = torch.rand(b, 3, h, w, generator=g)
    x = cond + torch.randn(b, 3, h, w, generator=g) * (50 / 255)
    return x, cond


def main():
    from fastdiffsr_amd.synth import state_dict_sha256, synth_nafnet
    arch, sde_utils = import_reference()
    torch.set_num_threads(8)
    out = {}
    for name, setting in (('test', TEST_SETTING), ('shipped', SHIPPED_SETTING)):
        net = arch.ConditionalNAFNet(img_channel=3, upscale=1, **setting)
        out['schema_' + name] = np.array(['%s %s' % (k, ','.join(map(str, v.shape))) for k, v in net.state_dict().items()])
    sd = synth_nafnet(0, **TEST_SETTING)
    out['synth_sha256'] = np.array(state_dict_sha256(sd))
    net = arch.ConditionalNAFNet(img_channel=3, upscale=1, **TEST_SETTING)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net.eval()

    # one forward at 36 x 44, int time, with every named tap (forward hooks on the reference's own sub-modules)
    x, cond = inputs(11, 2, 36, 44)
    taps = {}

    def hook(name):
        def fn(mod, args, res):
            taps[name] = (res[0] if isinstance(res, (list, tuple)) else res).detach()
        return fn
    hooks = [net.intro.register_forward_hook(hook('intro')), net.ending.register_forward_hook(hook('ending'))]
    hooks.append(net.enhance.register_forward_hook(lambda m, a, r: taps.__setitem__('enhance', (a[0] + r).detach())))
    for i, enc in enumerate(net.encoders):
        hooks += [blk.register_forward_hook(hook('encoders.%d.%d' % (i, j))) for j, blk in enumerate(enc)]
        hooks.append(net.downs[i].register_forward_hook(hook('downs.%d' % i)))
    hooks += [blk.register_forward_hook(hook('middle_blks.%d' % j)) for j, blk in enumerate(net.middle_blks)]
    for i, dec in enumerate(net.decoders):
        # ups.<i>: after "+ enc_skip" = the input of the decoder's first block
        hooks.append(dec[0].register_forward_pre_hook(lambda m, a, i=i: taps.__setitem__('ups.%d' % i, a[0][0].detach())))
        hooks += [blk.register_forward_hook(hook('decoders.%d.%d' % (i, j))) for j, blk in enumerate(dec)]
    with torch.no_grad():
        y = net(x, cond, 37)
    for h in hooks:
        h.remove()
    out.update(fwd_x=x.numpy(), fwd_cond=cond.numpy(), fwd_time=np.array(37), fwd_out=y.numpy())
    out['tap_names'] = np.array(list(taps))
    for k, v in taps.items():
        out['tap_' + k] = v.reshape(-1)[::TAP_STRIDE].numpy()
        out['tapshape_' + k] = np.array(v.shape)

    x2, cond2 = inputs(12, 2, 32, 32)
    t2 = torch.tensor([12.5, 77.25])
    with torch.no_grad():
        y2 = net(x2, cond2, t2)
    out.update(fwd2_x=x2.numpy(), fwd2_cond=cond2.numpy(), fwd2_time=t2.numpy(), fwd2_out=y2.numpy())

    for sched in ('cosine', 'linear', 'constant'):
        s = sde_utils.IRSDE(max_sigma=50, T=100, schedule=sched, eps=0.005, device='cpu')
        out.update({'sde_%s_thetas' % sched: s.thetas.numpy(), 'sde_%s_sigmas' % sched: s.sigmas.numpy(),
                    'sde_%s_sigma_bars' % sched: s.sigma_bars.numpy(), 'sde_%s_thetas_cumsum' % sched: s.thetas_cumsum.numpy(),
                    'sde_%s_dt' % sched: s.dt.numpy()})

    # a short loop: T 10, eps 0.5, explicit noise through a patched randn_like
    s = sde_utils.IRSDE(max_sigma=50, T=10, schedule='cosine', eps=0.5, device='cpu')
    s.set_model(net)
    x3, cond3 = inputs(13, 1, 32, 32)
    s.set_mu(cond3)
    noise = torch.randn(10, 1, 3, 32, 32, generator=torch.Generator().manual_seed(14))
    planes = list(noise)
    with torch.no_grad(), mock.patch.object(sde_utils.torch, 'randn_like', lambda t: planes.pop(0)):
        xs = s.reverse_sde(x3)
    with torch.no_grad():
        xo = s.reverse_ode(x3)
    out.update(loop_state=x3.numpy(), loop_cond=cond3.numpy(), loop_noise=noise.numpy(), loop_sde=xs.numpy(), loop_ode=xo.numpy())

    lq = torch.rand(2, 3, 9, 7, generator=torch.Generator().manual_seed(15))
    out.update(up_src=lq.numpy(), up_x4=torch.nn.functional.interpolate(lq, scale_factor=4, mode='bicubic').numpy())
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
