"""The test flow of MSI_SR_model/model/swinir.py (mfeNew_validateByClass) on the HIP engine:

    python -m fastdiffsr_amd.swinir.test --model generator_param.pkl (--hr DIR | --lr DIR) [--scale 4] -o OUT
                                         [--batch N] [--graph] [--max-images N]

DIR is a folder of images, or a folder of class folders (walked in sorted order, as the reference walks Test/).  With --hr the
LR input is made as the reference's TestDatasetFromFolder makes it -- the HR image cut down to a multiple of the scale, PIL
bicubic -- on the device (fdsr_resize_bicubic_u8, bit for bit Pillow's), and MSE / PSNR / SSIM / ERGAS of the SR image and of
the bicubic upscale beside it are computed on the device from the uint8 images and printed per class and overall.  With --lr
the images are super-resolved and written, nothing is scored.  SR PNGs carry save_img1's bytes ((x * 255) clamped, truncated).
One deliberate difference from the reference's metric path: it scores ToPILImage of the unclamped float output, which wraps
values outside [0, 1] around (mul(255).byte()); this path scores the clamped image it writes.
The architecture defaults to the reference's (embed_dim 180, 6 x 6 blocks, 6 heads, mlp_ratio 2); --embed-dim, --depths,
--num-heads, --mlp-ratio and --img-size describe another checkpoint."""
import argparse
import os

import numpy as np
import torch

from .. import metrics as M
from ..data import lr_to_sr
from .model import SwinIR, to_u8

EXTS = ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff')
FIELDS = ('mse', 'psnr', 'ssim', 'ergas')


def list_classes(root):
    """[(class name, [image paths])]: the class folders of root in sorted order, or root itself as one nameless class."""
    def images(d):
        return [os.path.join(d, n) for n in sorted(os.listdir(d)) if n.lower().endswith(EXTS)]
    dirs = [d for d in sorted(os.listdir(root)) if os.path.isdir(os.path.join(root, d))]
    if dirs:
        return [(d, images(os.path.join(root, d))) for d in dirs]
    return [('', images(root))]


def _read_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def _batches(paths, imgs, n):
    """Consecutive images of one size, at most n at a time."""
    i = 0
    while i < len(paths):
        j = i + 1
        while j < len(paths) and j - i < n and imgs[j].shape == imgs[i].shape:
            j += 1
        yield paths[i:j], np.stack(imgs[i:j])
        i = j


def run(model, classes, out_dir, scale, from_hr, batch=1, graph=False, max_images=None, log=print, label='SwinIR '):
    """The flow, for any model of this package that maps [B,3,h,w] in [0, 1] to [B,3,>=h*scale,>=w*scale] (fastdiffsr_amd.hat.test
    runs it too): the result is cut to (h*scale, w*scale) -- HAT, like its reference, returns the padded size."""
    from PIL import Image
    device = next(model.parameters()).device
    left = max_images if max_images is not None else float('inf')
    results, rows_all = {}, []
    for cls, paths in classes:
        paths = paths[:int(min(left, len(paths)))]
        left -= len(paths)
        if not paths:
            continue
        os.makedirs(os.path.join(out_dir, cls), exist_ok=True)
        imgs = [_read_rgb(p) for p in paths]
        if from_hr:
            imgs = [a[:a.shape[0] // scale * scale, :a.shape[1] // scale * scale] for a in imgs]
        rows = []
        for part, stack in _batches(paths, imgs, batch):
            u8 = torch.from_numpy(np.ascontiguousarray(stack)).to(device)
            if from_hr:
                hr_u8 = u8
                h, w = hr_u8.shape[1] // scale, hr_u8.shape[2] // scale
                lr, lr_u8 = lr_to_sr(hr_u8, h, w, want_u8=True)
                bic_u8 = lr_to_sr(lr_u8, h * scale, w * scale, want_u8=True)[1]
            else:
                lr_u8 = u8
            x = M.u8_to_tensor(lr_u8, min_max=(0, 1))                  # ToTensor()
            sr_u8 = to_u8(model(x, graph=graph)[:, :, :x.shape[2] * scale, :x.shape[3] * scale])
            if from_hr:
                sums = [M.image_metric_sums(t, hr_u8).cpu().numpy() for t in (sr_u8, bic_u8)]
                for i in range(len(part)):
                    sr, bic = (M.metrics_from_sums(s[i], tuple(hr_u8.shape[1:]), scale=scale) for s in sums)
                    rows.append({'sr': sr, 'bic': bic})
            host = sr_u8.cpu().numpy()
            for i, p in enumerate(part):
                Image.fromarray(host[i]).save(os.path.join(out_dir, cls, os.path.splitext(os.path.basename(p))[0] + '.png'))
        log('[%s] %d images' % (cls or '.', len(paths)))
        if rows:
            results[cls] = _report(rows, log, label)
            rows_all += rows
    if rows_all:
        log('[all] %d images' % len(rows_all))
        results['all'] = _report(rows_all, log, label)
    return results


def _report(rows, log, label='SwinIR '):
    out = {}
    for which, label in (('bic', 'Bicubic'), ('sr', label)):
        out[which] = {k: float(np.mean([r[which][k] for r in rows])) for k in FIELDS}
        log('  %s MSE %.4f  PSNR %.4f  SSIM %.4f  ERGAS %.4f' % ((label,) + tuple(out[which][k] for k in FIELDS)))
    return out


def _ints(s):
    return [int(v) for v in s.split(',')]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--model', required=True, help='generator.state_dict() as the reference saves it (generator_param.pkl)')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--hr', help='HR images: LR is made from them and the results are scored')
    src.add_argument('--lr', help='LR images: super-resolved and written')
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('-o', '--out', required=True)
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--graph', action='store_true', help='replay one captured graph per (batch, height, width)')
    ap.add_argument('--max-images', type=int, default=None)
    ap.add_argument('--embed-dim', type=int, default=180)
    ap.add_argument('--depths', type=_ints, default=[6] * 6)
    ap.add_argument('--num-heads', type=_ints, default=[6] * 6)
    ap.add_argument('--mlp-ratio', type=float, default=2.)
    ap.add_argument('--img-size', type=int, default=64, help='the img_size the checkpoint was built with (sizes its attn_mask buffers)')
    a = ap.parse_args(argv)
    device = torch.device('cuda', torch.cuda.current_device())
    model = SwinIR(upscale=a.scale, in_chans=3, img_size=a.img_size, window_size=8, img_range=1., depths=a.depths, embed_dim=a.embed_dim,
                   num_heads=a.num_heads, mlp_ratio=a.mlp_ratio, upsampler='pixelshuffle', resi_connection='1conv')
    sd = torch.load(a.model, map_location='cpu', weights_only=True)
    model.load_state_dict({k[7:] if k.startswith('module.') else k: v for k, v in sd.items()}, strict=True)
    model.to(device).eval()
    run(model, list_classes(a.hr or a.lr), a.out, a.scale, a.hr is not None, batch=a.batch, graph=a.graph, max_images=a.max_images)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
