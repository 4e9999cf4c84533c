"""The test flow of MSI_SR_model/model/hat.py (mfeNew_validateByClass) on the HIP engine:

    python -m fastdiffsr_amd.hat.test --model generator_param.pkl (--hr DIR | --lr DIR) [--scale 4] -o OUT
                                      [--batch N] [--graph] [--max-images N]

The flow is fastdiffsr_amd.swinir.test's (the reference's two files differ in the network's name): DIR is a folder of images
or of class folders; with --hr the LR input is made from the HR image as the reference's TestDatasetFromFolder makes it and
MSE / PSNR / SSIM / ERGAS of the SR image and of the bicubic upscale are printed per class and overall; with --lr the images
are super-resolved and written.  HAT returns the padded size times the scale, as its reference does: the command cuts the
result to (H * scale, W * scale) before it writes and scores.  The architecture defaults to the reference's (embed_dim 180,
6 x 6 HABs and one OCAB per group, 6 heads, window 16, mlp_ratio 4); --embed-dim, --depths, --num-heads, --mlp-ratio,
--squeeze-factor and --compress-ratio describe another checkpoint."""
import argparse

import torch

from ..swinir.test import _ints, list_classes, run
from .model import HAT


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
    ap.add_argument('--mlp-ratio', type=float, default=4.)
    ap.add_argument('--compress-ratio', type=int, default=3)
    ap.add_argument('--squeeze-factor', type=int, default=30)
    ap.add_argument('--img-size', type=int, default=64, help='the img_size the checkpoint was built with')
    a = ap.parse_args(argv)
    device = torch.device('cuda', torch.cuda.current_device())
    model = HAT(upscale=a.scale, in_chans=3, img_size=a.img_size, depths=a.depths, embed_dim=a.embed_dim, num_heads=a.num_heads,
                mlp_ratio=a.mlp_ratio, compress_ratio=a.compress_ratio, squeeze_factor=a.squeeze_factor)
    sd = torch.load(a.model, map_location='cpu', weights_only=True)
    model.load_state_dict({k[7:] if k.startswith('module.') else k: v for k, v in sd.items()}, strict=True)
    model.to(device).eval()
    run(model, list_classes(a.hr or a.lr), a.out, a.scale, a.hr is not None, batch=a.batch, graph=a.graph, max_images=a.max_images,
        label='HAT    ')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
