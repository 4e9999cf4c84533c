"""EDiffSR's config/sisr/test.py on the HIP engine, driven by the reference's own YAML options:

    python -m fastdiffsr_amd.ediffsr.test -opt setting_mfe_Test_x4.yml [--batch N] [--rng engine] [--seed S] [--graph]
                                          [--precision f32|f16x3|f16] [--results DIR] [--lpips BACKBONE.pth LIN.pth]

Reads `sde`, `degradation.scale`, `datasets.test*` (dataroot_GT / dataroot_LQ), `network_G.setting`, `path.pretrain_model_G`.
Per batch: LQ -> bicubic upscale on the device -> IRSDE.noise_state -> reverse_sde -> tensor2img (min_max (0, 1)) -> PSNR /
SSIM (11x11 Gaussian) / ERGAS [/ LPIPS] through the device metrics -> one RGB PNG per image -> the reference's log lines.
--rng engine draws x_T's noise and the per-step noise from the library's Philox stream at positions of the image's index in the
dataset, so the per-image results do not depend on --batch; --rng torch (default) draws from torch's generator like the reference.
--precision f16x3 runs the network's GEMMs on the fp32-grade f16 split (include/fdsr.h: fdsr_nafnet_set_precision); --precision
f16 keeps the activations as f16 in memory and takes one f16 MFMA per product (fdsr_nafnet_set_storage: PSNR-grade, not
fp32-grade).  Under either the range guard is read once per batch, and a batch that raised it is run again in f32 with a warning.
Single process.  Returns {dataset name: {'psnr', 'ssim', 'ergas', 'lpips', 'per_image', 'time'}}."""
import argparse
import logging
import os
import time

import numpy as np
import torch

from .. import _lib
from .. import metrics as M
from .model import ConditionalNAFNet, upscale
from .sde import IRSDE



def parse_options(path):
    import yaml
    with open(path) as f:
        opt = yaml.safe_load(f)
    for need in ('sde', 'degradation', 'datasets', 'network_G', 'path'):
        if need not in opt:
            raise KeyError('%s: missing section %r' % (path, need))
    opt['scale'] = opt['degradation']['scale']
    opt['datasets'] = {k: v for k, v in sorted(opt['datasets'].items()) if k.startswith('test')}
    return opt


def _read_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def _pairs(ds):
    names = sorted(n for n in os.listdir(ds['dataroot_LQ']) if n.lower().endswith(('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff')))
    gt = ds.get('dataroot_GT')
    return [(os.path.join(ds['dataroot_LQ'], n), os.path.join(gt, n) if gt else None) for n in names]


def build_model(opt, device):
    net = ConditionalNAFNet(**opt['network_G']['setting'])
    sd = torch.load(opt['path']['pretrain_model_G'], map_location='cpu', weights_only=True)
    net.load_state_dict({k[7:] if k.startswith('module.') else k: v for k, v in sd.items()}, strict=True)
    return net.to(device).eval()


def reverse_sde_guarded(net, sde, state, what, restore=None, **kwargs):
    """sde.reverse_sde(state, **kwargs) under the network's precision.  Under 'f16x3' / 'f16' the range guard is read once after
    the call, and a call that raised it is run again in f32 with a warning that names `what` (the images of the call); restore(),
    if given, first puts the caller's noise source back where it was before the call.  The network ends in the mode it had."""
    mode = net.precision
    sr = sde.reverse_sde(state, **kwargs)
    if mode in ('f16x3', 'f16'):
        try:
            net.check_saturation()
        except _lib.FdsrSaturated:
            logging.getLogger('fastdiffsr_amd.ediffsr').warning(
                '%s left the f16 range under --precision %s: running the batch again in f32', what, mode)
            net.set_precision('f32')
            if restore is not None:
                restore()
            sr = sde.reverse_sde(state, **kwargs)
            net.set_precision(mode)
    return sr


def run_dataset(opt, ds, net, sde, device, results, batch=1, rng='torch', seed=0, lpips=None, log=print):
    from PIL import Image
    scale, T = opt['scale'], opt['sde']['T']
    pairs = _pairs(ds)
    out_dir = os.path.join(results, ds['name'])
    os.makedirs(out_dir, exist_ok=True)
    per_image, times = [], []
    for b0 in range(0, len(pairs), batch):
        part = pairs[b0:b0 + batch]
        lq = M.u8_to_tensor(torch.from_numpy(np.stack([_read_rgb(p) for p, _ in part])).to(device), min_max=(0, 1))
        torch.cuda.synchronize(device)
        tic = time.time()
        mu = upscale(lq, scale)
        b, _, h, w = mu.shape
        if rng == 'engine':
            state = mu + net.randn(b, h, w, T, seed   # plane T: the steps use planes 0 .. T-1
                                     , first_image=b0, device=device) * sde.max_sigma
            sde.first_image = b0
        else:
            state = sde.noise_state(mu)
        sde.set_mu(mu)
        restore = None
        if net.precision in ('f16x3', 'f16') and rng == 'torch':
            rng_state = torch.cuda.get_rng_state(device)      # a re-run in f32 draws the same per-step noise
            restore = lambda: torch.cuda.set_rng_state(rng_state, device)   # noqa: E731
        sr = reverse_sde_guarded(net, sde, state, 'images %d..%d' % (b0, b0 + len(part) - 1), restore)
        sr_u8 = M.tensor2img_batch(sr, min_max=(0, 1))
        torch.cuda.synchronize(device)
        times.append((time.time() - tic) / len(part))
        rows = [{} for _ in part]
        if part[0][1] is not None:
            gt_u8 = torch.from_numpy(np.stack([_read_rgb(g) for _, g in part])).to(device)
            sums = M.image_metric_sums(sr_u8, gt_u8, gauss=True).cpu().numpy()
            lp = lpips.lpips_u8(gt_u8, sr_u8).cpu().numpy()[0, :, 0] if lpips is not None else [float('nan')] * len(part)
            for i in range(len(part)):
                m = M.metrics_from_sums(sums[i], tuple(sr_u8.shape[1:]), scale=scale)
                rows[i] = {'psnr': m['psnr'], 'ssim': m['ssim_gauss'], 'ergas': m['ergas'], 'lpips': float(lp[i])}
        host = sr_u8.cpu().numpy()
        for i, (p, _) in enumerate(part):
            name = os.path.splitext(os.path.basename(p))[0] + (opt.get('suffix') or '') + '.png'
            Image.fromarray(host[i]).save(os.path.join(out_dir, name))
            rows[i]['name'] = name
        per_image += rows
    res = {'per_image': per_image, 'time': float(np.mean(times))}
    for k in ('psnr', 'ssim', 'ergas', 'lpips'):
        res[k] = float(np.mean([r[k] for r in per_image])) if per_image and k in per_image[0] else float('nan')
    log('Test # PSNR: %0.5e, SSIM：%0.5e, ERGAS: %0.4e, LPIPS: %0.5e' % (res['psnr'], res['ssim'], res['ergas'], res['lpips']))
    log('average test time: %0.5e' % res['time'])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-opt', required=True, help='the reference\'s YAML test options')
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--rng', choices=('torch', 'engine'), default='torch')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--graph', action='store_true', help='replay one captured step')
    ap.add_argument('--precision', choices=ConditionalNAFNet.PRECISIONS, default='f32',
                    help='the GEMMs: exact fp32 (default), the fp32-grade f16 split, or f16 activations with one f16 MFMA per product')
    ap.add_argument('--results', default=None, help='output folder (default: results/<name> next to the options\' own tree)')
    ap.add_argument('--lpips', nargs=2, default=None, metavar=('BACKBONE', 'LIN'), help='AlexNet features and LPIPS v0.1 heads')
    a = ap.parse_args(argv)
    opt = parse_options(a.opt)
    device = torch.device('cuda', torch.cuda.current_device())
    net = build_model(opt, device)
    net.set_precision(a.precision)
    s = opt['sde']
    sde = IRSDE(max_sigma=s['max_sigma'], T=s['T'], schedule=s['schedule'], eps=s['eps'], device=device, rng=a.rng, graph=a.graph,
                seed=a.seed)
    sde.set_model(net)
    if a.rng == 'torch':
        torch.manual_seed(a.seed)
    lp = M.LPIPS(a.lpips[0], a.lpips[1], device=device) if a.lpips else None
    results = a.results or os.path.join('results', opt.get('name', 'ediffsr'))
    out = {}
    for _, ds in opt['datasets'].items():
        print('\nTesting [%s]...' % ds['name'])
        out[ds['name']] = run_dataset(opt, ds, net, sde, device, results, batch=a.batch, rng=a.rng, seed=a.seed, lpips=lp)
    return out


if __name__ == '__main__':
    main()
