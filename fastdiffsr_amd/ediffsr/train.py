"""EDiffSR's config/sisr/train.py on the HIP engine, driven by the reference's own YAML options:

    python -m fastdiffsr_amd.ediffsr.train -opt setting_mfe_Train_x4.yml [--batch N] [--seed S] [--root DIR] [--precision f32|f16]

Reads `sde`, `degradation.scale`, `datasets.train` / `datasets.val` (dataroot_GT / dataroot_LQ, GT_size, use_flip, use_rot,
batch_size), `network_G.setting`, `train.*`, `logger.print_freq` / `save_checkpoint_freq`, `path.pretrain_model_G` /
`resume_state`.  Per step: a batch of LQGT pairs (random GT_size crop with the aligned LQ crop, flip / rot), LQ -> bicubic
upscale on the device, IRSDE.generate_random_states, DenoisingModel.optimize_parameters, the lr update; a log line every
print_freq, a val pass (PSNR through ediffsr/test.py) every val_freq, `{iter}_G.pth` and `{iter}.state` every
save_checkpoint_freq under <root>/models and <root>/training_state (root: --root, else experiments/<name>).
--precision f16 trains with f16 activation storage and fp32 gradients; the val passes sample as they do under f32.  A
step whose forward leaves the f16 range is skipped; after MAX_CONSECUTIVE_SKIPS such steps in a row the run stops and names
--precision f32.  Single process; no EMA copy.  Returns {'losses', 'lrs', 'psnr', 'iter'}."""
import argparse
import os
import random

import numpy as np
import torch

from .denoising_model import DenoisingModel
from .model import upscale
from .sde import IRSDE
from . import test as T


MAX_CONSECUTIVE_SKIPS = 10


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-opt', required=True, help='the reference\'s YAML train options')
    ap.add_argument('--batch', type=int, default=None, help='overrides datasets.train.batch_size')
    ap.add_argument('--seed', type=int, default=None, help='overrides train.manual_seed')
    ap.add_argument('--root', default=None, help='experiment folder (default: experiments/<name>)')
    ap.add_argument('--precision', choices=('f32', 'f16'), default='f32',
                    help='storage of the activations training keeps: f32 (default) or f16 (mixed precision, fp32 gradients)')
    return ap


def parse_options(path):
    import yaml
    with open(path) as f:
        opt = yaml.safe_load(f)
    for need in ('sde', 'degradation', 'datasets', 'network_G', 'path', 'train'):
        if need not in opt:
            raise KeyError('%s: missing section %r' % (path, need))
    opt['scale'] = opt['degradation']['scale']
    opt['is_train'] = True
    return opt


def _augment(lq, gt, flip, rot):
    hflip = flip and random.random() < 0.5
    vflip = rot and random.random() < 0.5
    rot90 = rot and random.random() < 0.5
    out = []
    for img in (lq, gt):
        if hflip:
            img = img[:, ::-1, :]
        if vflip:
            img = img[::-1, :, :]
        if rot90:
            img = img.transpose(1, 0, 2)
        out.append(np.ascontiguousarray(img))
    return out


def _train_batch(ds, pairs, order, pos, batch, scale):
    lqs, gts = [], []
    gs = ds.get('GT_size')
    for k in range(batch):
        lp, gp = pairs[order[(pos + k) % len(order)]]
        lq, gt = T._read_rgb(lp), T._read_rgb(gp)
        if gs:
            ls = gs // scale
            y = random.randint(0, max(0, lq.shape[0] - ls))
            x = random.randint(0, max(0, lq.shape[1] - ls))
            lq = lq[y:y + ls, x:x + ls]
            gt = gt[y * scale:y * scale + gs, x * scale:x * scale + gs]
        lq, gt = _augment(lq, gt, ds.get('use_flip', False), ds.get('use_rot', False))
        lqs.append(lq)
        gts.append(gt)
    return np.stack(lqs), np.stack(gts)


def main(argv=None):
    from .. import metrics as M
    a = make_parser().parse_args(argv)
    opt = parse_options(a.opt)
    seed = a.seed if a.seed is not None else (opt['train'].get('manual_seed') or 0)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    root = a.root or os.path.join('experiments', opt.get('name', 'ediffsr'))
    opt['path'] = dict(opt['path'] or {}, models=os.path.join(root, 'models'), training_state=os.path.join(root, 'training_state'))
    for d in (opt['path']['models'], opt['path']['training_state']):
        os.makedirs(d, exist_ok=True)
    device = torch.device('cuda', torch.cuda.current_device())
    model = DenoisingModel(opt, train_precision=a.precision)
    s = opt['sde']
    sde = IRSDE(max_sigma=s['max_sigma'], T=s['T'], schedule=s['schedule'], eps=s['eps'], device=device)
    sde.set_model(model.model)
    scale, tr = opt['scale'], opt['train']
    ds = opt['datasets']['train']
    batch = a.batch or ds.get('batch_size', 1)
    pairs = T._pairs(ds)
    if not pairs:
        raise FileNotFoundError('no training pairs under %s' % ds['dataroot_LQ'])
    vds = opt['datasets'].get('val')
    step, epoch = 0, 0
    resume = opt['path'].get('resume_state')
    if resume:
        state = torch.load(resume, map_location='cpu', weights_only=False)
        g = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(resume))), 'models', '%d_G.pth' % state['iter'])
        model.model.load_state_dict(torch.load(g, map_location='cpu', weights_only=True), strict=True)
        model.resume_training(state)
        step, epoch = state['iter'], state['epoch']
        print('Resuming training from epoch: %d, iter: %d.' % (epoch, step))
    print_freq = (opt.get('logger') or {}).get('print_freq', 100)
    save_freq = (opt.get('logger') or {}).get('save_checkpoint_freq', 0)
    losses, lrs, psnrs = [], [], []
    order, pos = list(range(len(pairs))), len(pairs)
    while step < tr['niter']:
        if pos + batch > len(order):
            random.shuffle(order)
            pos = 0
            epoch += 1
        lq_u8, gt_u8 = _train_batch(ds, pairs, order, pos, batch, scale)
        pos += batch
        step += 1
        LQ = M.u8_to_tensor(torch.from_numpy(lq_u8).to(device), min_max=(0, 1))
        GT = M.u8_to_tensor(torch.from_numpy(gt_u8).to(device), min_max=(0, 1))
        LQ = upscale(LQ, scale)
        timesteps, states = sde.generate_random_states(x0=GT, mu=LQ)
        model.feed_data(states, LQ, GT)
        model.optimize_parameters(step, timesteps, sde)
        if model.consecutive_skips >= MAX_CONSECUTIVE_SKIPS:
            raise RuntimeError('iteration %d: %d steps in a row left the f16 range and were skipped; train this model with --precision f32'
                               % (step, model.consecutive_skips))
        lr_used = model.get_current_learning_rate()
        model.update_learning_rate(step, warmup_iter=tr.get('warmup_iter', -1))
        losses.append(model.get_current_log()['loss'])
        lrs.append(lr_used)
        if step % print_freq == 0:
            print('<epoch:%3d, iter:%8d, lr:%.3e> loss: %.4e' % (epoch, step, lr_used, losses[-1]))
        if vds and tr.get('val_freq') and step % tr['val_freq'] == 0:
            res = T.run_dataset(opt, dict(vds, name=vds.get('name', 'val')), model.model, sde, device, os.path.join(root, 'val_images'), batch=1,
                                log=lambda *_: None)
            psnrs.append((step, res['psnr']))
            print('<epoch:%3d, iter:%8d, psnr: %.6f' % (epoch, step, res['psnr']))
        if save_freq and step % save_freq == 0:
            print('Saving models and training states.')
            model.save(step)
            model.save_training_state(epoch, step)
    return {'losses': losses, 'lrs': lrs, 'psnr': psnrs, 'iter': step, 'opt_step': model.model.optim_state(model.model._names[0])[2],
            'skipped': model.skipped_steps}


if __name__ == '__main__':
    main()
